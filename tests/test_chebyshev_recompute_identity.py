"""The schedule the recomputed Chebyshev form rests on (ChebRecomputeF, csrc/vector.hip), on the numpy oracle alone.

The stored loop keeps the residual in memory across the smooth.  The recomputed one sends every operator product to a
buffer of its own (q0 = A x, q1 = A z1, q2 = A z2) and forms, per vector kernel, what it needs from b, the products and
dinv:

    K1:  z1 = c0 dinv (b - q0)
    K2:  r1 = (b - q0) - q1;  z2 = c1 z1 + c2 dinv r1           (z1 recomputed)
    K3:  r2 = r1 - q2;        z3 from z2 and r2;  x = ((x + z1) + z2) + z3      (optionally r2 and z3 are written)

with q0 absent from a zero guess (r0 = b, x is assigned) and one product fewer for k = 2.  The smoother's last operator
application is not issued: without a residual nobody reads it; in the fused mode the restriction forms
b - A x = r - A z from the r and z this schedule leaves.  No GPU."""
import numpy as np
import pytest

from oracle import pmg_oracle as po

TOL = 1e-12  # the bar of tests/test_fused_restriction_identity.py


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def coefficients(lmax, i):
    return (2.0 * i - 1.0) / (2.0 * i + 3.0), (8.0 * i + 4.0) / (2.0 * i + 3.0) / lmax


def recomputed_smooth(A, lmax, k, x, b, x_zero):
    """The recomputed schedule, kernel by kernel; every kernel reads only what the device kernel reads.
    Returns x and the (r, z) pair the fused mode hands to the restriction."""
    assert k in (2, 3)
    dinv = A.diag_inverse()
    c0 = 4.0 / (3.0 * lmax)
    q0 = None if x_zero else A.apply(x)

    def r0():
        return b.copy() if q0 is None else b - q0

    def k1():
        return c0 * dinv * r0()

    z1 = k1()  # K1 writes z1, the input of the next application
    q1 = A.apply(z1)

    def k2():
        r1 = r0() - q1
        c1, c2 = coefficients(lmax, 1)
        return r1, c1 * k1() + c2 * dinv * r1

    if k == 2:  # the final kernel over q0, q1
        r1, z2 = k2()
        z1 = k1()
        x = (z1 if x_zero else x + z1) + z2
        return x, r1, z2
    _, z2 = k2()  # K2 writes z2 alone
    q2 = A.apply(z2)
    r1, z2 = k2()  # K3 recomputes everything from b, q0, q1, q2 and dinv
    z1 = k1()
    r2 = r1 - q2
    c1, c2 = coefficients(lmax, 2)
    z3 = c1 * z2 + c2 * dinv * r2
    x = ((z1 if x_zero else x + z1) + z2) + z3
    return x, r2, z3


@pytest.fixture(scope="module")
def level():
    mesh = po.BoxMesh((3, 2, 4), warp=warp)
    P = 3
    A = po.Laplacian(P, 2.0, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P))
    eig, _ = po.estimate_eig_range(A, A.ndofs)
    rng = np.random.default_rng(5)
    b = rng.standard_normal(A.ndofs)
    b[A.bc.astype(bool)] = 0.0
    return A, eig, b, rng.standard_normal(A.ndofs)


@pytest.mark.parametrize("x_zero", [False, True], ids=["guess", "zero"])
@pytest.mark.parametrize("k", [2, 3])
def test_recomputed_schedule_reproduces_the_oracle_solve(level, k, x_zero):
    A, eig, b, x0 = level
    start = np.zeros_like(x0) if x_zero else x0
    sm = po.Chebyshev(eig, k)
    ref = sm.solve(A, start.copy(), b)
    got, r, z = recomputed_smooth(A, eig[1], k, start.copy(), b, x_zero)
    assert np.abs(got - ref).max() < TOL * np.abs(ref).max()
    # the fused mode: r - A z is the residual of the returned iterate (the oracle's last_residual has taken the last
    # application already, so it is b - A x itself)
    res = r - A.apply(z)
    assert np.abs(res - sm.last_residual).max() < TOL * np.abs(b).max()
    assert np.abs(res - (b - A.apply(ref))).max() < 10 * TOL * np.abs(b).max()


@pytest.mark.parametrize("k", [2, 3])
def test_a_zero_guess_is_the_guess_form_at_zero(level, k):
    """Assigning x (q0 absent) computes what the guess form computes from x = 0: A 0 = 0."""
    A, eig, b, x0 = level
    zero = np.zeros_like(x0)
    a = recomputed_smooth(A, eig[1], k, zero.copy(), b, True)
    g = recomputed_smooth(A, eig[1], k, zero.copy(), b, False)
    for u, v in zip(a, g):
        assert np.array_equal(u, v)
