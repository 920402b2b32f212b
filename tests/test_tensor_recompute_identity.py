"""The identities behind the recomputed tensor of the low-degree apply (TensorStream, GEO_RECOMPUTE, in
pmg-dolfinx_amd/csrc/stiffness_layer.hpp), in numpy alone: the eight monomial coefficient vectors of a trilinear cell
reproduce its vertex map, and the column form -- 15 values per (xi_a, eta_b), linear in zeta -- reproduces the oracle's
G at every GLL point of a twisted cell for P = 1, 2.

Bound 1e-14, relative to the largest entry of the point's tensor: both sides are a handful of products and sums of
O(1) numbers in FP64 (eps = 1.1e-16), followed by one division; a few tens of roundings at most."""
import numpy as np
import pytest

from oracle import pmg_oracle as po


def twisted_cell():
    """One genuinely trilinear cell (no two opposite faces parallel), vertex order k = 4 i + 2 j + l."""
    ref = np.array([[i, j, l] for i in (0, 1) for j in (0, 1) for l in (0, 1)], dtype=np.float64)
    x = ref * np.array([1.1, 0.9, 1.3])
    x[:, 0] += 0.12 * ref[:, 1] * ref[:, 2] + 0.07 * ref[:, 0] * ref[:, 1] * ref[:, 2]
    x[:, 1] += 0.10 * ref[:, 0] * ref[:, 2] - 0.05 * ref[:, 0] * ref[:, 1] * ref[:, 2]
    x[:, 2] += 0.08 * ref[:, 0] * ref[:, 1] + 0.06 * ref[:, 1] * ref[:, 2]
    return x + np.array([0.3, -0.2, 0.5])


def cell_coefficients(v):
    """c[4 i + 2 j + k] of x = sum c_ijk xi^i eta^j zeta^k, the differences cell_coefficient_kernel forms."""
    c = np.empty((8, 3))
    c[0] = v[0]
    c[1] = v[1] - v[0]
    c[2] = v[2] - v[0]
    c[3] = (v[3] - v[2]) - (v[1] - v[0])
    c[4] = v[4] - v[0]
    c[5] = (v[5] - v[4]) - (v[1] - v[0])
    c[6] = (v[6] - v[4]) - (v[2] - v[0])
    c[7] = ((v[7] - v[6]) - (v[5] - v[4])) - ((v[3] - v[2]) - (v[1] - v[0]))
    return c


def column_pieces(c, xi, eta, fold):
    """The 15 values of a column: dx/dxi and dx/deta at zeta = 0 with their slopes in zeta, and dx/dzeta, times fold."""
    e1 = c[3] + c[7] * xi
    return (fold * (c[4] + c[6] * eta), fold * (c[5] + c[7] * eta), fold * (c[2] + c[6] * xi), fold * e1,
            fold * (c[1] + c[5] * xi + e1 * eta))


def column_tensor(pieces, zeta, scale):
    """G at zeta from the pieces: J, adj(J), |det J|, adj adj^T scale / |det J| (adjugate and metric of laplacian.hpp)."""
    a0, a1, b0, b1, cz = pieces
    J = np.stack([a0 + zeta * a1, b0 + zeta * b1, cz], axis=1)  # J[i][d] = d x_i / d xi_d
    K = np.empty((3, 3))
    K[0, 0] = J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]
    K[0, 1] = -J[0, 1] * J[2, 2] + J[0, 2] * J[2, 1]
    K[0, 2] = J[0, 1] * J[1, 2] - J[0, 2] * J[1, 1]
    K[1, 0] = -J[1, 0] * J[2, 2] + J[1, 2] * J[2, 0]
    K[1, 1] = J[0, 0] * J[2, 2] - J[0, 2] * J[2, 0]
    K[1, 2] = -J[0, 0] * J[1, 2] + J[0, 2] * J[1, 0]
    K[2, 0] = J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]
    K[2, 1] = -J[0, 0] * J[2, 1] + J[0, 1] * J[2, 0]
    K[2, 2] = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
    det = abs(J[0, 0] * K[0, 0] + J[0, 1] * K[1, 0] + J[0, 2] * K[2, 0])
    M = K @ K.T * (scale / det)
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def test_coefficients_reproduce_the_vertex_map():
    v = twisted_cell()
    c = cell_coefficients(v)
    for i in (0, 1):
        for j in (0, 1):
            for l in (0, 1):
                mono = np.array([(i ** a) * (j ** b) * (l ** d) for a in (0, 1) for b in (0, 1) for d in (0, 1)], float)
                got = mono @ c
                assert np.abs(got - v[4 * i + 2 * j + l]).max() < 1e-14 * np.abs(v).max()
    # ... and the map between the vertices: the trilinear interpolant at an interior point
    p = np.array([0.3, 0.6, 0.8])
    shape = np.array([(p[0] if i else 1 - p[0]) * (p[1] if j else 1 - p[1]) * (p[2] if l else 1 - p[2])
                      for i in (0, 1) for j in (0, 1) for l in (0, 1)])
    mono = np.array([(p[0] ** a) * (p[1] ** b) * (p[2] ** d) for a in (0, 1) for b in (0, 1) for d in (0, 1)])
    assert np.abs(mono @ c - shape @ v).max() < 1e-14 * np.abs(v).max()


@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("P", [1, 2])
def test_column_form_reproduces_the_tensor(P, reflect):
    v = twisted_cell()
    if reflect:  # a left-handed local frame: xi reversed
        v = v[[4, 5, 6, 7, 0, 1, 2, 3]]
    nd = P + 1
    pts, w = po.gll_points_weights(nd)
    dphi, w3 = po.geometry_tables(P)
    G, _ = po.geometry_G(v, np.arange(8, dtype=np.int32)[None, :], dphi, w3)
    c = cell_coefficients(v)
    worst = 0.0
    for a in range(nd):
        for b in range(nd):
            pieces = column_pieces(c, pts[a], pts[b], w[a] * w[b])  # (the weights folded: G is homogeneous of degree 1 in J)
            assert sum(p.size for p in pieces) == 15
            for k in range(nd):
                got = column_tensor(pieces, pts[k], w[k])
                want = G[0, (a * nd + b) * nd + k]
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f"column form against the oracle's G, P = {P}, reflected {reflect}: {worst:.3e}")
    assert worst < 1e-14
