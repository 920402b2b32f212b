"""Numpy reference for the coefficient-tensor tests (tests/test_coefficient_tensor_abi.py,
tests/test_gpu_coefficient_tensor.py): the stored tensor of -div(kappa kq K grad u) with K symmetric positive definite
and constant per cell, G_q = adj(J) K_c adj(J)^T w_q / det J, written with adj(J) = det(J) J^-1 through numpy.linalg --
nothing of the library's or the oracle's adjugate code -- and the tensors the tests and the drivers use."""
import numpy as np

from oracle import pmg_oracle as po

ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # (xx, xy, xz, yy, yz, zz), the order of G


def full(T):
    """[n, 6] -> [n, 3, 3] symmetric."""
    T = np.asarray(T, dtype=np.float64)
    M = np.empty(T.shape[:-1] + (3, 3))
    for d, (i, j) in enumerate(ORDER):
        M[..., i, j] = M[..., j, i] = T[..., d]
    return M


def packed(M):
    """[n, 3, 3] symmetric -> [n, 6]."""
    return np.ascontiguousarray(np.stack([M[..., i, j] for i, j in ORDER], axis=-1))


def tensor_G(P, xgeom, geom_dofmap, T):
    """[ncells][nq][6]: the six entries of adj(J) K_c adj(J)^T w_q / det J at every quadrature point, with
    J[d, r] = d x_d / d xi_r of the trilinear map and K_c = full(T[c])."""
    dphi, w3 = po.geometry_tables(P)  # [3, nq, 8], [nq]
    xc = np.asarray(xgeom)[np.asarray(geom_dofmap)]  # [nc, 8, 3]
    J = np.einsum("ckd,rqk->cqdr", xc, dphi)
    det = np.linalg.det(J)
    adj = det[..., None, None] * np.linalg.inv(J)  # [nc, nq, r, d]
    # |det J|: a left-handed cell (det J < 0) has the same positive-definite tensor as in any other frame
    M = np.einsum("cqad,cde,cqbe->cqab", adj, full(T), adj) * (w3[None, :] / np.abs(det))[..., None, None]
    return packed(M)


def laplacian(P, kappa, dofmap, xgeom, geom_dofmap, bc_marker):
    """An oracle ``po.Laplacian`` that remembers its mesh (the oracle's class keeps only the tensor made from it), so
    that ``with_tensor`` can write the tensor anew."""
    A = po.Laplacian(P, kappa, dofmap, xgeom, geom_dofmap, bc_marker)
    A.xgeom, A.geom_dofmap = np.asarray(xgeom), np.asarray(geom_dofmap)
    return A


def with_tensor(A, T, kq=None):
    """The oracle operator ``A`` (from ``laplacian`` above) turned into that of -div(kappa kq K grad u): its stored
    tensor replaced by ``tensor_G``, scaled by the nodal field at each point's dof when one is given, its cached
    diagonal dropped.  Returns ``A``."""
    A.G = tensor_G(A.P, A.xgeom, A.geom_dofmap, T)
    if kq is not None:
        A.G = A.G * np.asarray(kq)[A.dofmap][:, :, None]
    A._diag = None
    return A


def rotating_tensor(centres):
    """The drivers' tensor: eigenvalues (1, 2 + x, 4), rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre."""
    c = np.asarray(centres, dtype=np.float64)
    n = c.shape[0]
    az, ax = 0.6 + 0.8 * c[:, 1], 0.4 + 0.5 * c[:, 2]
    Rz = np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(az), -np.sin(az), np.sin(az), np.cos(az), 1.0
    Rx = np.zeros((n, 3, 3))
    Rx[:, 0, 0], Rx[:, 1, 1], Rx[:, 1, 2], Rx[:, 2, 1], Rx[:, 2, 2] = 1.0, np.cos(ax), -np.sin(ax), np.sin(ax), np.cos(ax)
    R = Rz @ Rx
    lam = np.stack([np.ones(n), 2.0 + c[:, 0], np.full(n, 4.0)], axis=1)
    return packed(np.einsum("nij,nj,nkj->nik", R, lam, R))


def random_spd(ncells, seed):
    """Seeded tensors with eigenvalues in [0.5, 2] and a random rotation each; all three off-diagonals non-zero (a
    rotation that leaves one below 1e-3 is drawn again), so no component order or sign can hide."""
    rng = np.random.default_rng(seed)
    out = np.empty((ncells, 6))
    for c in range(ncells):
        while True:
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            M = (Q * rng.uniform(0.5, 2.0, 3)) @ Q.T
            M = 0.5 * (M + M.T)
            if min(abs(M[0, 1]), abs(M[0, 2]), abs(M[1, 2])) > 1e-3:
                break
        out[c] = packed(M)
    return out


def cell_centres(xgeom, geom_dofmap):
    """The mean of each cell's eight vertices, [ncells, 3]."""
    return np.asarray(xgeom)[np.asarray(geom_dofmap)].mean(axis=1)
