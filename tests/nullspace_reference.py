"""CPU restatement of the constant-null-space solvers (pmg_vec_remove_mean, pmg_cg_set_nullspace,
pmg_amg_set_nullspace), in numpy.  TEST INFRASTRUCTURE ONLY; pinned from first principles in
tests/test_nullspace_reference.py.

With N the number of dofs, 1 the vector of ones and Pi = I - 1 1^T / N:

  * ``remove_mean``: x - sum(x) / N, or with weights x - (w . x) / (w . 1) -- the mean is a quotient;
  * ``pcg_nullspace``: r_0 = Pi (b - A x_0); z = M r; rz = r . z - (1 . r)(1 . z) / N; p = Pi z + beta p;
    alpha = rz / (p . y); stop on rz / rz_0 < rtol^2; x <- Pi x after the loop.  The flexible variant takes
    beta = r_new . (Pi z_new - Pi z_old) / rz_old;
  * ``coarsest_inverse``: v = P_{L-2}^T ... P_0^T 1, gamma = max diag(A_c) / (v^T v), inv(A_c + gamma v v^T);
  * ``NullspaceAmgCycle``: the V(k, k) cycle of ``oracle.amg_oracle.AmgCycle`` with that inverse on the last level
    (a copy of its few lines: AmgCycle's constructor inverts the singular matrix)."""
import numpy as np


def remove_mean(x, w=None):
    x = np.asarray(x, dtype=np.float64)
    if w is None:
        return x - x.sum() / x.size
    return x - (w @ x) / w.sum()


def projected_rz(rz, sum_r, sum_z, N):
    return rz - (sum_r * sum_z) / N


def pcg_nullspace(A_apply, M_apply, b, x0, rtol, max_iter, flexible=False):
    """Returns (x, iterations).  ``M_apply(r)`` is the preconditioner; None = the identity."""
    M = M_apply if M_apply is not None else (lambda r: r.copy())
    N = b.size
    x = np.array(x0, dtype=np.float64)
    r = remove_mean(b - A_apply(x))
    z = M(r)
    rz0 = rz = projected_rz(r @ z, r.sum(), z.sum(), N)
    p = z - z.sum() / N
    z_old, sz_old = z, z.sum()
    its = 0
    while rz0 != 0.0 and its < max_iter:
        its += 1
        y = A_apply(p)
        alpha = rz / (p @ y)
        x = x + alpha * p
        r = r - alpha * y
        z = M(r)
        sr, sz = r.sum(), z.sum()
        rz_new = projected_rz(r @ z, sr, sz, N)
        sub = projected_rz(r @ z_old, sr, sz_old, N) if flexible else 0.0
        beta = (rz_new - sub) / rz
        z_old, sz_old = z, sz
        rz = rz_new
        if rz / rz0 < rtol * rtol:
            break
        p = beta * p + (z - sz / N)
    return remove_mean(x), its


def restricted_ones(Ps, n0):
    v = np.ones(n0)
    for P in Ps:
        v = P.T @ v
    return v


def coarsest_inverse(As, Ps):
    """(inverse of A_c + gamma v v^T, v, gamma) for the hierarchy (As, Ps)."""
    Ac = As[-1].toarray()
    v = restricted_ones(Ps, As[0].shape[0])
    gamma = Ac.diagonal().max() / (v @ v)
    return np.linalg.inv(Ac + gamma * np.outer(v, v)), v, gamma


class NullspaceAmgCycle:
    """``oracle.amg_oracle.AmgCycle`` with ``coarsest_inverse`` on the last level.  ``cycle`` is the bare V-cycle (the
    preconditioner of the projected CG); ``cycle_projected`` and ``stationary`` end with the mean removed, as
    pmg_amg_cycle and the stationary solve do."""

    def __init__(self, As, Ps, lmax, k=2):
        from oracle import pmg_oracle as po
        from oracle.amg_oracle import _CsrOp

        self.As, self.Ps, self.k = As, Ps, k
        self.ops = [_CsrOp(A) for A in As]
        self.smoothers = [po.Chebyshev((0.0, lm), k) for lm in lmax]
        self.dense, self.v, self.gamma = coarsest_inverse(As, Ps)

    def cycle(self, b, l=0):
        if l == len(self.As) - 1:
            return self.dense @ b
        A, P = self.As[l], self.Ps[l]
        x = self.smoothers[l].solve(self.ops[l], np.zeros_like(b), b)
        xc = self.cycle(P.T @ (b - A @ x), l + 1)
        x = x + P @ xc
        return self.smoothers[l].solve(self.ops[l], x, b)

    def cycle_projected(self, b):
        return remove_mean(self.cycle(b))

    def stationary(self, b, cycles):
        x = self.cycle(b)
        for _ in range(1, cycles):
            x = x + self.cycle(b - self.As[0] @ x)
        return remove_mean(x)

    def pcg(self, A_apply, b, rtol, max_iter):
        """The Krylov mode: projected CG from x = 0 with the bare cycle as the preconditioner."""
        return pcg_nullspace(A_apply, self.cycle, b, np.zeros_like(b), rtol, max_iter)
