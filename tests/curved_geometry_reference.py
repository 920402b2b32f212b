"""Numpy reference for the curved-cell tests (tests/test_curved_geometry_reference.py, tests/test_curved_geometry_abi.py,
tests/test_gpu_curved_geometry.py): the coordinate element of degree g (tensor-product Lagrange on the GLL nodes, nodes
in ascending tensor order), an oracle operator whose stored tensor comes from it, and the quantities the existing
``*_reference.py`` modules fix to 8 nodes, restated from J itself: mass weights, facet weights, the tensor-coefficient
G.  Everything is built from the oracle's 1-D tables; nothing of the library's code."""
import numpy as np

from oracle import pmg_oracle as po

ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---- tables ---------------------------------------------------------------------------------------------------------

def tables_1d(P, g):
    """(L, Lp) [nd, g+1]: the 1-D basis of the coordinate element and its derivative at the GLL points of degree P."""
    xi, _ = po.gll_points_weights(P + 1)
    if g == 1:
        return np.stack([1.0 - xi, xi], axis=1), np.stack([-np.ones(P + 1), np.ones(P + 1)], axis=1)
    nodes, _ = po.gll_points_weights(g + 1)
    L = po.lagrange_eval_matrix(nodes, xi)
    # l_i'(x) = sum_k l_k(x) l_i'(node_k): the derivative of a degree-g polynomial, interpolated exactly
    return L, L @ po.lagrange_deriv_matrix(nodes)


def tables(P, g):
    """``dphi_geometry`` [3, nq, (g+1)^3] and the 3-D GLL weights [nq]: ``oracle.geometry_tables`` for any g."""
    nd, m = P + 1, g + 1
    _, w = po.gll_points_weights(nd)
    L, Lp = tables_1d(P, g)
    dx = np.einsum("ai,bj,cl->abcijl", Lp, L, L).reshape(nd**3, m**3)
    dy = np.einsum("ai,bj,cl->abcijl", L, Lp, L).reshape(nd**3, m**3)
    dz = np.einsum("ai,bj,cl->abcijl", L, L, Lp).reshape(nd**3, m**3)
    w3 = np.einsum("a,b,c->abc", w, w, w).ravel()
    return np.ascontiguousarray(np.stack([dx, dy, dz], axis=0)), np.ascontiguousarray(w3)


def corners(g):
    """Positions of the 8 corners k = i*4 + j*2 + l among the (g+1)^3 nodes."""
    m = g + 1
    return np.array([((i * g) * m + j * g) * m + l * g for i in (0, 1) for j in (0, 1) for l in (0, 1)])


def jacobians(P, g, xgeom, geom_dofmap):
    """J[c, q, d, r] = d x_d / d xi_r by the dense table."""
    dphi, _ = tables(P, g)
    return np.einsum("ckd,rqk->cqdr", np.asarray(xgeom)[np.asarray(geom_dofmap)], dphi)


def jacobians_sum_factorised(P, g, xgeom, geom_dofmap):
    """The same J by the three 1-D contractions in the cell-cooperative kernel's order, as explicit loops: along z with
    L and L', then along y, then along x; every sum runs over its index in ascending order."""
    nd, m = P + 1, g + 1
    L, Lp = tables_1d(P, g)
    X = np.asarray(xgeom)[np.asarray(geom_dofmap)].reshape(-1, m, m, m, 3)  # [c, i, j, l, d]
    nc = X.shape[0]
    A0 = np.zeros((nc, m, m, nd, 3))
    A1 = np.zeros((nc, m, m, nd, 3))
    for c in range(nd):
        for l in range(m):
            A0[:, :, :, c] += L[c, l] * X[:, :, :, l]
            A1[:, :, :, c] += Lp[c, l] * X[:, :, :, l]
    B0 = np.zeros((nc, m, nd, nd, 3))
    B1 = np.zeros((nc, m, nd, nd, 3))
    B2 = np.zeros((nc, m, nd, nd, 3))
    for b in range(nd):
        for j in range(m):
            B0[:, :, b] += L[b, j] * A0[:, :, j]
            B1[:, :, b] += Lp[b, j] * A0[:, :, j]
            B2[:, :, b] += L[b, j] * A1[:, :, j]
    J = np.zeros((nc, nd, nd, nd, 3, 3))
    for a in range(nd):
        for i in range(m):
            J[:, a, :, :, :, 0] += Lp[a, i] * B0[:, i]
            J[:, a, :, :, :, 1] += L[a, i] * B1[:, i]
            J[:, a, :, :, :, 2] += L[a, i] * B2[:, i]
    return J.reshape(nc, nd**3, 3, 3)


# ---- the operator and the quantities around it ----------------------------------------------------------------------

def laplacian(P, g, kappa, dofmap, xgeom, geom_dofmap, marker):
    """An oracle ``Laplacian`` constructed on the 8 corners, then given the stored tensor and the determinant of the
    degree-g geometry.  It remembers its mesh (``with_tensor``)."""
    gd = np.asarray(geom_dofmap)
    A = po.Laplacian(P, kappa, dofmap, xgeom, gd[:, corners(g)], marker)
    dphi, w3 = tables(P, g)
    A.G, A.detJ = po.geometry_G(np.asarray(xgeom), gd, dphi, w3)
    A._diag = None
    A.g, A.xgeom, A.geom_dofmap = g, np.asarray(xgeom), gd
    return A


def tensor_G(P, g, xgeom, geom_dofmap, T):
    """adj(J) K_c adj(J)^T w_q / |det J| with adj(J) = det(J) J^-1 through numpy.linalg, K_c symmetric [ncells, 6]."""
    _, w3 = tables(P, g)
    J = jacobians(P, g, xgeom, geom_dofmap)
    det = np.linalg.det(J)
    adj = det[..., None, None] * np.linalg.inv(J)
    Kc = np.empty((len(T), 3, 3))
    for d, (i, j) in enumerate(ORDER):
        Kc[:, i, j] = Kc[:, j, i] = np.asarray(T)[:, d]
    M = np.einsum("cqad,cde,cqbe->cqab", adj, Kc, adj) * (w3[None, :] / np.abs(det))[..., None, None]
    return np.ascontiguousarray(np.stack([M[..., i, j] for i, j in ORDER], axis=-1))


def with_tensor(A, T=None, kq=None):
    """``A`` (from ``laplacian``) as the operator of -div(kappa kq K grad u); T None: no tensor.  Returns ``A``."""
    if T is None:
        dphi, w3 = tables(A.P, A.g)
        A.G, _ = po.geometry_G(A.xgeom, A.geom_dofmap, dphi, w3)
    else:
        A.G = tensor_G(A.P, A.g, A.xgeom, A.geom_dofmap, T)
    if kq is not None:
        A.G = A.G * np.asarray(kq)[A.dofmap][:, :, None]
    A._diag = None
    return A


def mass_weights(P, g, xgeom, geom_dofmap):
    """w_q |det J_q| [ncells, nq]."""
    _, w3 = tables(P, g)
    return w3[None, :] * np.abs(np.linalg.det(jacobians(P, g, xgeom, geom_dofmap)))


def mass_vector(P, g, coeff, dofmap, xgeom, geom_dofmap, marker, f=None):
    """sum over the points on a dof of coeff_c w_q |det J_q| (f[dof]); 0 on marked dofs: the load vector (coeff =
    kappa, f given) and the reaction vector (coeff = sigma)."""
    dm = np.asarray(dofmap, dtype=np.int64)
    wts = mass_weights(P, g, xgeom, geom_dofmap) * np.asarray(coeff, dtype=np.float64).reshape(-1, 1)
    if f is not None:
        wts = wts * np.asarray(f)[dm]
    d = np.bincount(dm.ravel(), weights=wts.ravel(), minlength=len(marker))
    d[np.asarray(marker).astype(bool)] = 0.0
    return d


def facet_nodes(P, lf):
    nd = P + 1
    axis, side = lf // 2, lf % 2
    idx = [np.arange(nd)] * 3
    idx[axis] = np.array([P if side else 0])
    a, b, c = np.meshgrid(*idx, indexing="ij")
    return ((a * nd + b) * nd + c).ravel()


def facet_weights(P, g, xgeom, geom_dofmap, cells, facets):
    """w1[i] w1[j] |row ``axis`` of adj(J)| per facet point [nfacets, nd^2], adj(J) = det(J) J^-1."""
    nd = P + 1
    _, w = po.gll_points_weights(nd)
    w2 = np.outer(w, w).ravel()
    cells = np.asarray(cells, dtype=np.int64)
    J = jacobians(P, g, xgeom, np.asarray(geom_dofmap)[cells])
    out = np.empty((cells.size, nd * nd))
    for F, lf in enumerate(np.asarray(facets, dtype=np.int64)):
        Jf = J[F][facet_nodes(P, int(lf))]
        adj = np.linalg.det(Jf)[:, None, None] * np.linalg.inv(Jf)
        out[F] = w2 * np.linalg.norm(adj[:, int(lf) // 2, :], axis=1)
    return out


def facet_vector(P, g, dofmap, xgeom, geom_dofmap, cells, facets, values, marker):
    """sum over facet points on a dof of w2 |dS| value; 0 on marked dofs: the Neumann load and the Robin face mass."""
    wds = facet_weights(P, g, xgeom, geom_dofmap, cells, facets)
    dm = np.asarray(dofmap, dtype=np.int64)
    dofs = np.stack([dm[c][facet_nodes(P, int(lf))] for c, lf in zip(cells, facets)])
    d = np.bincount(dofs.ravel(), weights=(wds * np.asarray(values).reshape(wds.shape)).ravel(), minlength=len(marker))
    d[np.asarray(marker).astype(bool)] = 0.0
    return d


# ---- maps -----------------------------------------------------------------------------------------------------------

def quarter_annulus(x):
    """(r cos t, r sin t, z) with r = 1 + x, t = pi y / 2: 1 <= r <= 2, height 1, volume 3 pi / 4."""
    r, t = 1.0 + x[:, 0], 0.5 * np.pi * x[:, 1]
    return np.stack([r * np.cos(t), r * np.sin(t), x[:, 2]], axis=1)


def triquadratic(x):
    """A degree-2 element holds it exactly."""
    return np.stack([x[:, 0] + 0.15 * x[:, 1] ** 2, x[:, 1] + 0.1 * x[:, 2] * x[:, 0], x[:, 2] + 0.1 * x[:, 0] ** 2],
                    axis=1)


def box_mesh(n, g, warp=None, per_cell=False):
    """(xgeom, geom_dofmap [ncells, (g+1)^3]) of the unit box with n cells per axis, cells lexicographic (x slowest) as
    ``oracle.BoxMesh``: the degree-g GLL nodes of every cell, mapped by ``warp``.  Shared nodes are stored once, or
    once per cell with ``per_cell``."""
    n = (n,) * 3 if np.isscalar(n) else tuple(n)
    m = g + 1
    xi, _ = po.gll_points_weights(m)
    lines = []
    for a in range(3):
        v = np.linspace(0.0, 1.0, n[a] + 1)
        lines.append(np.concatenate([(v[:-1, None] + xi[None, :-1] * (v[1:, None] - v[:-1, None])).ravel(), v[-1:]]))
    X, Y, Z = np.meshgrid(*lines, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    shape = [n[a] * g + 1 for a in range(3)]
    cx, cy, cz = [c.ravel() for c in np.meshgrid(*[np.arange(k) for k in n], indexing="ij")]
    gd = np.empty((cx.size, m**3), dtype=np.int32)
    for i in range(m):
        for j in range(m):
            for l in range(m):
                gd[:, (i * m + j) * m + l] = ((cx * g + i) * shape[1] + (cy * g + j)) * shape[2] + cz * g + l
    if per_cell:
        x, gd = x[gd.ravel()], np.arange(gd.size, dtype=np.int32).reshape(gd.shape)
    if warp is not None:
        x = warp(x)
    return np.ascontiguousarray(x), gd


def onto_the_sphere(x, r0=0.4):
    """The cube [-1, 1]^3 of ``multiblock_mesh.ogrid`` with its outer blocks pushed onto the unit sphere: a point at
    cube radius s = max |x_i| > r0 stays on its ray and gets the radius (1 - t) |x| r0 / s + t, t = (s - r0) / (1 - r0)
    -- between the ray's point on the inner cube's surface (t = 0) and its point on the sphere (t = 1), monotone in t
    because the former is at most sqrt(3) r0 < 1.  The inner cube stays, the faces s = 1 land on |x| = 1.  A function
    of position alone (shared nodes stay shared), smooth inside every cell (the kinks lie on the diagonal planes
    between the blocks)."""
    s = np.abs(x).max(axis=1)
    rho = np.maximum(np.linalg.norm(x, axis=1), 1e-300)
    t = np.clip((s - r0) / (1.0 - r0), 0.0, 1.0)
    radius = np.where(s > r0, (1.0 - t) * rho * r0 / np.maximum(s, 1e-300) + t, rho)
    return x * (radius / rho)[:, None]


def multiblock_nodes(mesh, g, warp=None, per_cell=True):
    """Degree-g arrays of a ``multiblock_mesh.MultiblockMesh``: the nodes of each cell at the trilinear positions of its
    own frame, then mapped by ``warp``.  Shared nodes are stored once per cell, or once (``per_cell=False``: nodes that
    coincide before the map are merged)."""
    x, gd = trilinear_nodes(mesh.xgeom, mesh.geom_dofmap, g)
    if not per_cell:
        _, first, inverse = np.unique(np.round(x, 10), axis=0, return_index=True, return_inverse=True)
        x, gd = x[first], np.asarray(inverse).reshape(gd.shape).astype(np.int32)
    if warp is not None:
        x = warp(x)
    return np.ascontiguousarray(x), np.ascontiguousarray(gd)


def trilinear_nodes(xgeom, corner_dofmap, g):
    """Degree-g arrays (one node set per cell) whose nodes sit at the trilinear positions of each cell's own 8 corners:
    the same geometry as the degree-1 mesh, exactly representable at any g."""
    m = g + 1
    xi, _ = po.gll_points_weights(m)
    phi = np.stack([1.0 - xi, xi], axis=1)
    N = np.einsum("ai,bj,cl->abcijl", phi, phi, phi).reshape(m**3, 8)
    x = np.einsum("tk,ckd->ctd", N, np.asarray(xgeom)[np.asarray(corner_dofmap)]).reshape(-1, 3)
    return np.ascontiguousarray(x), np.arange(x.shape[0], dtype=np.int32).reshape(-1, m**3)
