"""Numpy reference for the Robin-term tests (tests/test_robin_abi.py, tests/test_gpu_robin.py): the operator of
-div(K grad u) + sigma u with the boundary condition K grad u . n + alpha u = g on listed facets.  The weak form gains
int_Gamma alpha u v ds; with GLL collocation the face quadrature points are the face nodes, so that face mass matrix is
diagonal, d_R[dof] = sum over the listed facets' points on the dof of w1[i] w1[j] |dS| alpha, zero on marked dofs.  The
surface weights are tests/boundary_data_reference.py's (adj(J) through numpy.linalg, nothing of the library's or the
oracle's geometry code); the diffusion part is the oracle's Laplacian and the reaction vector is
tests/reaction_reference.py's.  tests/test_robin_abi.py pins d_R by solving two manufactured problems exactly."""
import numpy as np

import boundary_data_reference as bd
import reaction_reference as rr
from oracle import pmg_oracle as po


def robin_vector(part, P, dofmap, cells, facets, alpha, bc_marker, ndofs=None):
    """d_R over the dofs of ``bc_marker``: ``alpha`` [nfacets, nd*nd] holds one value per facet point, in the order of
    ``boundary_data_reference.facet_nodes_axes``."""
    ndofs = np.asarray(bc_marker).shape[0] if ndofs is None else ndofs
    if len(cells) == 0:
        return np.zeros(ndofs)
    wds, _ = bd.facet_geometry(part, P, cells, facets)
    dofs = bd.facet_dofs(P, np.asarray(dofmap).reshape(-1, (P + 1) ** 3), cells, facets)
    d = np.bincount(dofs.ravel(), weights=(wds * np.asarray(alpha, dtype=np.float64).reshape(wds.shape)).ravel(),
                    minlength=ndofs)
    d[np.asarray(bc_marker).astype(bool)] = 0.0
    return d


class RobinLaplacian:
    """``A`` (an oracle ``po.Laplacian``, or anything with its members) plus d_sigma + d_R.  It has the members the
    oracle's Chebyshev, CG and multigrid classes and ``amg_oracle`` use (apply, diagonal, diag_inverse, assemble_csr,
    ndofs, dofmap, bc)."""

    def __init__(self, A, d_R, d_sigma=None):
        self.A = A
        self.P, self.nd, self.ndofs, self.dofmap, self.bc = A.P, A.nd, A.ndofs, A.dofmap, A.bc
        self.d_R = np.asarray(d_R, dtype=np.float64)
        self.d_sigma = np.zeros(A.ndofs) if d_sigma is None else np.asarray(d_sigma, dtype=np.float64)
        self.d = self.d_sigma + self.d_R  # in that order, as the library sums them

    def apply(self, u, cells=None):
        assert cells is None
        u = np.asarray(u, dtype=np.float64)
        return self.A.apply(u) + self.d * u  # d is zero on the marked rows: they stay y = x

    def diagonal(self):
        return self.A.diagonal() + self.d

    def diag_inverse(self):
        return 1.0 / self.diagonal()

    def assemble_csr(self):
        import scipy.sparse as sp

        return (self.A.assemble_csr() + sp.diags(self.d)).tocsr()

    def dense(self):
        return self.assemble_csr().toarray()


def laplacian(part, P, kappa, dofmap, bc_marker, cells, facets, alpha, sigma=None):
    """The oracle's scalar operator on ``part`` with the Robin term of (cells, facets, alpha) and, optionally, the
    reaction term of ``sigma``."""
    A = po.Laplacian(P, kappa, dofmap, part.xgeom, part.geom_dofmap, bc_marker)
    d_sigma = None if sigma is None else rr.reaction_vector(P, sigma, dofmap, part.xgeom, part.geom_dofmap, bc_marker)
    return RobinLaplacian(A, robin_vector(part, P, dofmap, cells, facets, alpha, bc_marker), d_sigma)


def random_alpha(nfacets, nf, seed):
    """Seeded values in [0, 4] per facet point, about a fifth exactly 0."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 4.0, (nfacets, nf))
    a[rng.uniform(size=a.shape) < 0.2] = 0.0
    return a


def linear_alpha(A):
    """The drivers' coefficient alpha = A (1 + y), as a callable of the facet-point coordinates."""
    return lambda pts: A * (1.0 + np.asarray(pts)[:, 1])


def one_face_marker(bc_marker, coords, axis=0):
    """The marker restricted to the face x_axis = 0 of the box."""
    return (np.asarray(bc_marker).astype(bool) & (np.abs(coords[:, axis]) < 1e-12)).astype(np.int8)


# ---- the manufactured problems: the unit box, kappa = 2, boundary_data_reference.exact ------------------------------

FACE_ALPHA = (0.0, 0.7, 1.9, 0.0, 3.1, 0.4)  # one constant per box face, local facets 0..5
FACE_ALPHA_NO_DIRICHLET = (1.1, 0.7, 1.9, 0.0, 3.1, 0.4)


def manufactured_problem(part, P, face_alpha, dirichlet_on_x0):
    """(u, b, d_R, marker, K): the nodal exact solution, the right-hand side of the unconstrained problem -- volume
    load plus int_Gamma g v ds with g = kappa grad u . n + alpha u per facet point through the Neumann reference --,
    the face-mass diagonal, the marker (x = 0 or empty) and the unconstrained dense stiffness matrix."""
    lv = part.level(P)
    cells, facets = part.exterior_facets()
    coords = part.dof_coordinates(P)
    u, gr, lap = bd.exact(P)
    nd = P + 1
    marker = one_face_marker(lv.bc_marker, coords) if dirichlet_on_x0 else np.zeros(lv.ndofs, dtype=np.int8)
    alpha = np.repeat(np.asarray(face_alpha, dtype=np.float64)[facets.astype(int)][:, None], nd * nd, axis=1)
    _, normal = bd.facet_geometry(part, P, cells, facets)
    dofs = bd.facet_dofs(P, lv.dofmap, cells, facets)
    pts = coords[dofs.ravel()]
    g = (bd.KAPPA * np.einsum("fsd,fsd->fs", gr(pts).reshape(dofs.shape + (3,)), normal)
         + alpha * u(pts).reshape(dofs.shape))
    A = po.Laplacian(P, bd.KAPPA, lv.dofmap, part.xgeom, part.geom_dofmap, np.zeros(lv.ndofs, dtype=np.int8))
    Ae = A.element_matrices()
    K = np.zeros((lv.ndofs, lv.ndofs))
    for c in range(part.ncells):
        K[np.ix_(A.dofmap[c], A.dofmap[c])] += Ae[c]
    nomark = np.zeros(lv.ndofs, dtype=np.int8)
    b = np.bincount(A.dofmap.ravel(), weights=(bd.KAPPA * A.w3[None, :] * A.detJ * (-lap(coords))[A.dofmap]).ravel(),
                    minlength=lv.ndofs)
    b += bd.neumann_reference(part, P, lv.dofmap, cells, facets, g, nomark, lv.ndofs)
    d_R = robin_vector(part, P, lv.dofmap, cells, facets, alpha, nomark)
    return u(coords), b, d_R, marker, K


def dense_solve(u, b, d, marker, K):
    """Lift the marked values of u, solve the unmarked rows of (K + diag(d)) x = b."""
    marked = np.asarray(marker).astype(bool)
    M = K + np.diag(d)
    rhs = b - M @ np.where(marked, u, 0.0)
    x = u.copy()
    free = ~marked
    x[free] = np.linalg.solve(M[np.ix_(free, free)], rhs[free])
    return x, M
