"""Numpy reference for the boundary-data tests (tests/test_boundary_data_abi.py, tests/test_gpu_boundary_data.py):
the surface element and the Neumann load written down from the trilinear map itself -- adj(J) = det(J) J^-1 through
numpy.linalg, nothing of the library's or the oracle's geometry code -- and the mixed problem whose discrete solution
is the exact one."""
import numpy as np

from oracle import pmg_oracle as po


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def facet_nodes_axes(P, local_facet):
    """(t, i, j): cell-local node numbers of the face and their 1-D indices along the two remaining axes, written
    independently of pmg_dolfinx_amd.mesh.facet_nodes (which the tests compare against it)."""
    nd = P + 1
    axis, side = local_facet // 2, local_facet % 2
    t, ii, jj = [], [], []
    for i in range(nd):
        for j in range(nd):
            abc = [i, j]
            abc.insert(axis, P if side else 0)
            t.append((abc[0] * nd + abc[1]) * nd + abc[2])
            ii.append(i)
            jj.append(j)
    return np.array(t), np.array(ii), np.array(jj)


def facet_geometry(part, P, cells, facets):
    """For each listed facet and face point: area weight w1[i] w1[j] |dS| and the outward unit normal.
    dS n = det(J) J^-T N with N = +-e_axis the reference normal (Nanson), i.e. +- row `axis` of adj(J)."""
    nd = P + 1
    xi, w = po.gll_points_weights(nd)
    nf = len(cells)
    wds = np.zeros((nf, nd * nd))
    normal = np.zeros((nf, nd * nd, 3))
    for F, (c, lf) in enumerate(zip(cells, facets)):
        axis, side = int(lf) // 2, int(lf) % 2
        t, ii, jj = facet_nodes_axes(P, int(lf))
        xc = part.xgeom[part.geom_dofmap[c]]  # [8, 3], vertex k = i*4 + j*2 + l
        for s in range(nd * nd):
            abc = [ii[s], jj[s]]
            abc.insert(axis, P if side else 0)
            r = xi[abc]  # reference coordinates of the point
            ph = np.stack([1.0 - r, r], axis=1)  # [3 axes, 2]
            dp = np.array([-1.0, 1.0])
            J = np.zeros((3, 3))  # J[d, a] = d x_d / d xi_a
            for i in range(2):
                for j in range(2):
                    for l in range(2):
                        k = i * 4 + j * 2 + l
                        grad = np.array([dp[i] * ph[1, j] * ph[2, l], ph[0, i] * dp[j] * ph[2, l],
                                         ph[0, i] * ph[1, j] * dp[l]])
                        J += np.outer(xc[k], grad)
            adj = np.linalg.det(J) * np.linalg.inv(J)
            row = adj[axis]
            ds = np.linalg.norm(row)
            wds[F, s] = w[ii[s]] * w[jj[s]] * ds
            normal[F, s] = (1.0 if side else -1.0) * row / ds
    return wds, normal


def facet_dofs(P, dofmap, cells, facets):
    return np.stack([dofmap[c][facet_nodes_axes(P, int(lf))[0]] for c, lf in zip(cells, facets)])


def neumann_reference(part, P, dofmap, cells, facets, h, marker, ndofs, size_local=None):
    """b[i] = sum over facet points with dof i of w2 |dS| h, unmarked owned rows only."""
    wds, _ = facet_geometry(part, P, cells, facets)
    dofs = facet_dofs(P, dofmap, cells, facets)
    b = np.bincount(dofs.ravel(), weights=(wds * np.asarray(h).reshape(wds.shape)).ravel(), minlength=ndofs)
    b[np.asarray(marker).astype(bool)] = 0.0
    if size_local is not None:
        b[size_local:] = 0.0
    return b


# ---- the mixed problem: Dirichlet on x = 0, x = 1, y = 0, Neumann on y = 1, z = 0, z = 1 of the unit box -----------

KAPPA = 2.0


def exact(P):
    """(u, grad u, laplace u) as functions of coordinates [n, 3]; degree <= P - 1 per variable, so the GLL rule
    integrates every term of the weak form exactly and the discrete solution is u at the nodes."""
    if P >= 3:
        u = lambda c: 1.3 + c[:, 0] ** 2 * c[:, 1] - c[:, 2] ** 2 + 3 * c[:, 0] * c[:, 2] + 0.5 * c[:, 1]  # noqa: E731
        gr = lambda c: np.stack([2 * c[:, 0] * c[:, 1] + 3 * c[:, 2], c[:, 0] ** 2 + 0.5,  # noqa: E731
                                 -2 * c[:, 2] + 3 * c[:, 0]], axis=1)
        lap = lambda c: 2 * c[:, 1] - 2.0  # noqa: E731
    else:
        u = lambda c: 1.3 + c[:, 0] * c[:, 1] - 2 * c[:, 2] + 3 * c[:, 0] * c[:, 2]  # noqa: E731
        gr = lambda c: np.stack([c[:, 1] + 3 * c[:, 2], c[:, 0], -2.0 + 3 * c[:, 0]], axis=1)  # noqa: E731
        lap = lambda c: np.zeros(c.shape[0])  # noqa: E731
    return u, gr, lap


def dirichlet_part(c):
    return (np.abs(c[:, 0]) < 1e-12) | (np.abs(c[:, 0] - 1.0) < 1e-12) | (np.abs(c[:, 1]) < 1e-12)


def mixed_problem_data(part, P, cells, facets):
    """Nodal u, f / kappa (what assemble_rhs takes), the flux h = kappa grad u . n per facet point, the marker."""
    lv = part.level(P)
    coords = part.dof_coordinates(P)
    u, gr, lap = exact(P)
    marker = (lv.bc_marker.astype(bool) & dirichlet_part(coords)).astype(np.int8)
    _, normal = facet_geometry(part, P, cells, facets)
    dofs = facet_dofs(P, lv.dofmap, cells, facets)
    g = gr(coords[dofs.ravel()]).reshape(dofs.shape + (3,))
    h = KAPPA * np.einsum("fsd,fsd->fs", g, normal)
    return u(coords), -lap(coords), h, marker
