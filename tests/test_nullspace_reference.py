"""tests/nullspace_reference.py pinned from first principles, without a GPU.

1. The projected CG on the oracle's operator with an all-zero marker (3^3 cells, P = 2, warped: 343 dofs): the dense
   matrix is built column by column, A 1 = 0, and ``pcg_nullspace`` with the Jacobi preconditioner reproduces
   x* = pinv(A) b -- also from a right-hand side and from an initial guess with a constant added.
   A deviation from the tolerance rule the GPU tests use (|x - x*| / |x*| <= 10 e_ref + 1e-12 with e_ref the
   restatement's own error): here the restatement IS what is tested, and the rule applied to it is circular.
   The bound instead: the iteration stops on sqrt(rz / rz_0) < rtol, the M^-1-norm of the residual; the error in x is at most
   cond(D^-1 A on the complement of the constants) times that, so the bound is kappa_eff * rtol with kappa_eff computed
   from the dense matrix.
2. ``coarsest_inverse`` on hierarchies of the restated set-up (oracle.amg_oracle.build) of the unmarked degree-1 matrix,
   one level (6^3 cells, 343 rows) and two (10^3 cells, 1331 rows; level 1 exactly singular): a coarse right-hand side
   restricted from a mean-free fine residual is solved exactly, the solution is orthogonal to v, and the perturbed
   matrix has a Cholesky factorisation."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as bd  # noqa: E402
import nullspace_reference as ns  # noqa: E402

RTOL = 1e-12


def unmarked_operator(n, P, warp, kappa=2.0):
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh(n, warp=warp)
    return mesh, po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, np.zeros(mesh.ndofs(P), np.int8))


@pytest.fixture(scope="module")
def dense_case():
    mesh, A = unmarked_operator(3, 2, bd.warp)
    n = A.ndofs
    assert n == 343
    M = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        M[:, j] = A.apply(e)
        e[j] = 0.0
    b = np.random.default_rng(11).standard_normal(n)
    b -= b.mean()
    x_star = np.linalg.pinv(M, hermitian=True) @ b
    d = M.diagonal()
    lam = np.linalg.eigvalsh(M / np.sqrt(np.outer(d, d)))
    kappa_eff = lam[-1] / lam[1]  # lam[0] is the null space
    return A, M, b, x_star, kappa_eff


def test_remove_mean_is_a_quotient():
    x = np.random.default_rng(1).integers(-8, 9, 1000).astype(np.float64)
    assert np.array_equal(ns.remove_mean(x), x - x.sum() / x.size)
    w = np.random.default_rng(2).uniform(0.5, 1.5, 1000)
    y = ns.remove_mean(x, w)
    assert abs(w @ y) <= 1000 * 2.0 ** -53 * np.abs(w).max() * np.abs(x).max() * 4
    assert abs(ns.remove_mean(x).sum()) <= 1000 * 2.0 ** -53 * np.abs(x).max()


def test_the_unmarked_operator_is_singular_on_the_constants(dense_case):
    A, M, b, x_star, kappa_eff = dense_case
    assert np.abs(M @ np.ones(M.shape[0])).max() <= 1e-13 * np.abs(M).max()
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
    lam = np.linalg.eigvalsh(M)
    assert abs(lam[0]) <= 1e-12 * lam[-1] and lam[1] > 1e-6 * lam[-1]  # the constants are the whole null space


@pytest.mark.parametrize("shift_b,shift_x0", [(0.0, 0.0), (0.7, 0.0), (0.0, 3.5), (-2.0, 1.25)])
def test_projected_cg_reproduces_the_pseudo_inverse(dense_case, shift_b, shift_x0):
    A, M, b, x_star, kappa_eff = dense_case
    dinv = A.diag_inverse()
    x0 = np.full(b.size, shift_x0)
    x, its = ns.pcg_nullspace(A.apply, lambda r: dinv * r, b + shift_b, x0, RTOL, 2000)
    err = np.linalg.norm(x - x_star) / np.linalg.norm(x_star)
    print(f"b + {shift_b}, x0 = {shift_x0}: {its} iterations, |x - x*| / |x*| = {err:.3e}, "
          f"kappa_eff = {kappa_eff:.3e}, bound {kappa_eff * RTOL:.3e}")
    assert 0 < its < 2000
    assert err <= kappa_eff * RTOL
    assert abs(x.sum()) <= x.size * 2.0 ** -53 * np.abs(x).max()


def test_flexible_variant_agrees_for_a_fixed_preconditioner(dense_case):
    A, M, b, x_star, kappa_eff = dense_case
    dinv = A.diag_inverse()
    x, its = ns.pcg_nullspace(A.apply, lambda r: dinv * r, b, np.zeros_like(b), RTOL, 2000, flexible=True)
    assert np.linalg.norm(x - x_star) / np.linalg.norm(x_star) <= kappa_eff * RTOL


def test_plain_cg_drifts_or_diverges_where_the_projected_one_does_not(dense_case):
    """What the mode is for: with a constant in b the plain recurrences of the oracle's CG never reach the tolerance."""
    from oracle import pmg_oracle as po

    A, M, b, x_star, kappa_eff = dense_case
    cg = po.CGSolver()
    cg.set_max_iterations(400)
    cg.set_tolerance(RTOL)
    x = np.zeros_like(b)
    try:
        with np.errstate(all="ignore"):
            its = cg.solve(A, x, b + 0.7)
    except ZeroDivisionError:  # p has become a (huge) constant: p . A p = 0
        its = None
    err = np.linalg.norm(ns.remove_mean(x) - x_star) / np.linalg.norm(x_star)
    print(f"plain CG on b + 0.7: {its} iterations, error of the mean-free part {err:.3e}")
    assert its is None or its == 400 or not np.isfinite(err) or err > kappa_eff * RTOL


@pytest.fixture(scope="module", params=[(6, 1), (10, 2)], ids=["one-level", "two-levels"])
def hierarchy(request):
    from oracle import amg_oracle as ao

    n, levels = request.param
    mesh, A = unmarked_operator(n, 1, bd.warp)
    As, Ps, rhos, _ = ao.build(A.assemble_csr())
    assert len(As) == levels and As[0].shape[0] == (n + 1) ** 3
    return As, Ps, rhos


def test_coarsest_inverse_solves_what_the_cycle_restricts(hierarchy):
    As, Ps, rhos = hierarchy
    inv, v, gamma = ns.coarsest_inverse(As, Ps)
    Ac = As[-1].toarray()
    np.linalg.cholesky(Ac + gamma * np.outer(v, v))  # raises if not positive definite
    r = np.random.default_rng(5).standard_normal(As[0].shape[0])
    r -= r.mean()
    bc = r
    for P in Ps:
        bc = P.T @ bc
    x = inv @ bc
    res = np.linalg.norm(Ac @ x - bc) / np.linalg.norm(bc)
    orth = abs(v @ x) / (np.linalg.norm(v) * np.linalg.norm(x))
    print(f"{len(As)} level(s), coarsest {Ac.shape[0]} rows: |A_c x - b_c| / |b_c| = {res:.3e}, "
          f"|v . x| / (|v| |x|) = {orth:.3e}, gamma = {gamma:.3e}")
    assert res <= 1e-10 and orth <= 1e-10
    if not Ps:
        assert np.array_equal(v, np.ones(Ac.shape[0]))


def test_restated_cycle_is_a_preconditioner_for_the_projected_cg(hierarchy):
    As, Ps, rhos = hierarchy
    cyc = ns.NullspaceAmgCycle(As, Ps, rhos)
    A0 = As[0]
    b = np.random.default_rng(6).standard_normal(A0.shape[0])
    b -= b.mean()
    x, its = cyc.pcg(lambda p: A0 @ p, b, 1e-10, 60)
    res = np.linalg.norm(A0 @ x - b) / np.linalg.norm(b)
    print(f"{len(As)} level(s): AMG-PCG {its} iterations, |A x - b| / |b| = {res:.3e}")
    assert its < 30 and res < 1e-8
    assert abs(cyc.cycle_projected(b).sum()) <= b.size * 2.0 ** -53 * np.abs(cyc.cycle(b)).max()
