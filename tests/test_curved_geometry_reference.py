"""The curved-cell reference (tests/curved_geometry_reference.py) pinned on the CPU before it judges any kernel: its
tables against the oracle's and the library's, exactly representable geometry at several degrees, the convergence of
the quarter annulus' volume with the geometry degree, and the dense Jacobian against its sum-factorised form -- the
spread of the latter is the yardstick of the GPU tensor's bound (profiles/curved_geometry.md)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import curved_geometry_reference as cg  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402


@pytest.mark.parametrize("P", [1, 2, 4])
def test_degree_one_tables_are_the_oracles(P):
    dphi, w3 = cg.tables(P, 1)
    ref_dphi, ref_w3 = po.geometry_tables(P)
    assert np.array_equal(dphi, ref_dphi) and np.array_equal(w3, ref_w3)


@pytest.mark.parametrize("order", ["ascending", "basix", "custom"])
@pytest.mark.parametrize("P,g", [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 3), (6, 3), (8, 4), (5, 4)])
def test_library_table_equals_the_reference(built, P, g, order):
    import pmg_dolfinx_amd as pm

    perm = np.random.default_rng(P).permutation(P + 1).astype(np.int32) if order == "custom" else None
    got = pm.coordinate_element_table(P, g, node_order=order, perm1d=perm)
    p1 = pm.node_permutation(order, P, perm)
    want = cg.tables(P, g)[0][:, pm.cell_permutation(p1), :]  # the caller's row q = ascending row perm3[q]
    err = np.abs(got - want).max()
    print(f"P = {P}, g = {g}, {order}: max |table - reference| = {err:.2e} (entries up to {np.abs(want).max():.1f})")
    assert got.shape == (3, (P + 1) ** 3, (g + 1) ** 3)
    assert err < 1e-14  # (the library's GLL points and numpy's differ in the last bit at some degrees)


@pytest.mark.parametrize("P", [2, 4])
def test_triquadratic_box_is_exact_from_degree_two(P):
    n = (2, 3, 2)
    G = {}
    for g in (1, 2, 3, 4):
        x, gd = cg.box_mesh(n, g, warp=cg.triquadratic)
        G[g], _ = po.geometry_G(x, gd, *cg.tables(P, g))
    scale = np.abs(G[2]).max()
    for g in (3, 4):
        err = np.abs(G[g] - G[2]).max() / scale
        print(f"P = {P}: G at g = {g} against g = 2: {err:.2e}")
        assert err < 1e-13
    away = np.abs(G[1] - G[2]).max() / scale
    print(f"P = {P}: G at g = 1 against g = 2: {away:.2e} (negative control)")
    assert away > 1e-3


def annulus_volume_error(P, g, n=(2, 3, 2), per_cell=False):
    x, gd = cg.box_mesh(n, g, warp=cg.quarter_annulus, per_cell=per_cell)
    return abs(cg.mass_weights(P, g, x, gd).sum() - 0.75 * np.pi) / (0.75 * np.pi)


def test_annulus_volume_converges_with_the_geometry_degree():
    err = {g: annulus_volume_error(4, g) for g in (1, 2, 3, 4)}
    print("quarter annulus, 2 x 3 x 2 cells, P = 4: relative volume error "
          + ", ".join(f"g = {g}: {e:.2e}" for g, e in err.items()))
    for g in (1, 2, 3):
        assert err[g] > 100 * err[g + 1], (g, err)
    assert annulus_volume_error(4, 2, per_cell=True) == pytest.approx(err[2], rel=1e-9)


SPREAD_CASES = [(1, 2), (2, 2), (3, 2), (4, 2), (6, 2), (1, 3), (2, 3), (3, 3), (4, 3), (6, 3), (8, 4)]


@pytest.mark.parametrize("P,g", SPREAD_CASES)
def test_dense_jacobian_equals_the_sum_factorised_one(P, g):
    """The two differ in the order of their sums only: (g+1)^3 terms against three sums of g + 1.  The sum itself is
    not well conditioned -- the derivative table has entries up to 13 at g = 4 and alternating signs, so
    S = sum_k |x_k| |dphi_k| is many times |J| -- and the standard bound for two orders of one dot product is
    |J_dense - J_sf| <= (n_dense + n_sf + 4) eps S (n terms each, two roundings per table product on either side).
    The tensor adj(J) adj(J)^T / det J is a rational function of J with relative condition at most 6 cond(J) (three
    factors, two-norm), which bounds its spread by that of J.  The worst relative spread per (P, g) is printed;
    profiles/curved_geometry.md records it and the GPU test's bound for the exported tensor is made from it."""
    x, gd = cg.box_mesh((2, 3, 2), g, warp=cg.quarter_annulus)
    Jd, Js = cg.jacobians(P, g, x, gd), cg.jacobians_sum_factorised(P, g, x, gd)
    sj = np.abs(Jd - Js).max() / np.abs(Jd).max()
    S = np.einsum("ckd,rqk->cqdr", np.abs(x[gd]), np.abs(cg.tables(P, g)[0])).max()
    bound_j = ((g + 1) ** 3 + 3 * (g + 1) + 4) * np.finfo(float).eps * S / np.abs(Jd).max()
    bound_g = 6 * np.linalg.cond(Jd).max() * bound_j

    def G_of(J):
        det = np.linalg.det(J)
        adj = det[..., None, None] * np.linalg.inv(J)
        return np.einsum("cqad,cqbd->cqab", adj, adj) / np.abs(det)[..., None, None]

    Gd, Gs = G_of(Jd), G_of(Js)
    sg = np.abs(Gd - Gs).max() / np.abs(Gd).max()
    print(f"P = {P}, g = {g}: spread of J {sj:.2e} (bound {bound_j:.1e}), of adj adj^T / det {sg:.2e} "
          f"(bound {bound_g:.1e})")
    assert sj < bound_j and sg < bound_g
