"""Numpy reference for the reaction-term tests (tests/test_reaction_abi.py, tests/test_gpu_reaction.py): the operator
of -div(K grad u) + sigma u with sigma constant per cell.  With GLL collocation the quadrature points are the nodes, so
the mass matrix is diagonal and the term is one vector, d[dof] = sum over the cells' points on the dof of
sigma_c w_q |det J_q|, zero on marked dofs; the operator is y = A x + d x on unmarked rows and y = x on marked ones.
The diffusion part is the oracle's Laplacian (with whatever tensor or field the caller has written into it:
tests/tensor_coefficient_reference.py); the determinant here comes from numpy.linalg, not from the oracle's or the
library's cofactor code.  tests/test_reaction_abi.py pins d against the mass matrix written down from the weak form."""
import numpy as np

from oracle import pmg_oracle as po


def mass_weights(P, xgeom, geom_dofmap):
    """[ncells, nq]: w_q |det J_q| of the trilinear map at the GLL points."""
    dphi, w3 = po.geometry_tables(P)  # [3, nq, 8], [nq]
    xc = np.asarray(xgeom)[np.asarray(geom_dofmap)]  # [nc, 8, 3]
    J = np.einsum("ckd,rqk->cqdr", xc, dphi)
    return np.abs(np.linalg.det(J)) * w3[None, :]


def reaction_vector(P, sigma, dofmap, xgeom, geom_dofmap, bc_marker, cells=None):
    """d over the dofs of ``bc_marker``; ``cells`` (optional) restricts the sum to those cells."""
    nd = P + 1
    dm = np.asarray(dofmap, dtype=np.int64).reshape(-1, nd**3)
    wd = mass_weights(P, xgeom, geom_dofmap) * np.asarray(sigma, dtype=np.float64)[:, None]
    if cells is not None:
        dm, wd = dm[cells], wd[cells]
    d = np.zeros(np.asarray(bc_marker).shape[0])
    np.add.at(d, dm.ravel(), wd.ravel())
    d[np.asarray(bc_marker).astype(bool)] = 0.0
    return d


class ReactionLaplacian:
    """``A`` (an oracle ``po.Laplacian``) plus the reaction vector of ``sigma``.  It has the members the oracle's
    Chebyshev, CG and multigrid classes use (apply, diag_inverse, ndofs, dofmap, bc)."""

    def __init__(self, A, sigma, xgeom, geom_dofmap):
        self.A = A
        self.P, self.nd, self.ndofs, self.dofmap, self.bc = A.P, A.nd, A.ndofs, A.dofmap, A.bc
        self.d = reaction_vector(A.P, sigma, A.dofmap, xgeom, geom_dofmap, A.bc)

    def apply(self, u, cells=None):
        assert cells is None
        u = np.asarray(u, dtype=np.float64)
        return self.A.apply(u) + self.d * u  # d is zero on the marked rows: they stay y = x

    def diagonal(self):
        return self.A.diagonal() + self.d  # marked rows: 1 + 0

    def diag_inverse(self):
        return 1.0 / self.diagonal()

    def assemble_csr(self):
        import scipy.sparse as sp

        return (self.A.assemble_csr() + sp.diags(self.d)).tocsr()

    def dense(self):
        """The dense matrix (tiny meshes only)."""
        return self.assemble_csr().toarray()


def laplacian(P, kappa, sigma, dofmap, xgeom, geom_dofmap, bc_marker):
    """The oracle's scalar operator plus the reaction term."""
    return ReactionLaplacian(po.Laplacian(P, kappa, dofmap, xgeom, geom_dofmap, bc_marker), sigma, xgeom, geom_dofmap)


def random_sigma(ncells, seed):
    """Seeded values in [0, 4], about a fifth of the cells exactly 0."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 4.0, ncells)
    s[rng.uniform(size=ncells) < 0.2] = 0.0
    return s


def linear_sigma(S):
    """The drivers' coefficient sigma_c = S (1 + x_c), as a callable of the cell centres."""
    return lambda centres: S * (1.0 + np.asarray(centres)[:, 0])
