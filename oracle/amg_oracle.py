"""CPU restatement of the library's algebraic multigrid (``csrc/amg.hip``): the solve phase (``AmgCycle``) and the
set-up (``aggregate``, ``smoothed_prolongator``, ``power_bound``, ``build``).

TEST INFRASTRUCTURE ONLY.  The reference's coarse solver is PETSc KSPCG + hypre BoomerAMG
(``src/amg.hpp:33-47``) -- third-party arithmetic with no fixture, so parity with the reference is
unpinned for this component.  What is pinned here: given the SAME hierarchy (the matrices and
prolongators the library exports, themselves checked against first principles in
``tests/test_gpu_amg.py``: A_0 against the oracle's assembled operator, A_{l+1} = P^T A_l P), the
device cycle must equal this numpy/scipy cycle -- V(k, k) with the 4th-kind Chebyshev / Jacobi
smoother of ``src/chebyshev.hpp:46-91`` (the oracle's own ``Chebyshev``), exact solve on the last
level.  And the hierarchy itself: what the library exports must equal the set-up restated in the
second half of this file, level by level (``tests/test_gpu_amg_setup.py``,
``tests/test_gpu_amg_distributed_setup.py``; the restatement alone: ``tests/test_amg_oracle.py``)."""
from __future__ import annotations

import numpy as np


class _CsrOp:
    """What oracle.pmg_oracle.Chebyshev.solve needs of an operator."""

    def __init__(self, A):
        self.A = A
        self._dinv = 1.0 / A.diagonal()

    def apply(self, x):
        return self.A @ x

    def diag_inverse(self):
        return self._dinv


class AmgCycle:
    def __init__(self, As, Ps, lmax, k=2):
        from . import pmg_oracle as po

        self.As, self.Ps, self.k = As, Ps, k
        self.ops = [_CsrOp(A) for A in As]
        self.smoothers = [po.Chebyshev((0.0, lm), k) for lm in lmax]
        self.dense = np.linalg.inv(As[-1].toarray())

    def cycle(self, b, l=0):
        """x = M b, one V(k, k) cycle from a zero initial guess."""
        if l == len(self.As) - 1:
            return self.dense @ b
        A, P = self.As[l], self.Ps[l]
        x = self.smoothers[l].solve(self.ops[l], np.zeros_like(b), b)
        xc = self.cycle(P.T @ (b - A @ x), l + 1)
        x = x + P @ xc
        return self.smoothers[l].solve(self.ops[l], x, b)

    def stationary(self, b, cycles):
        """The stationary solve of ``cycles`` cycles: x = M b, then x += M (b - A_0 x)."""
        x = self.cycle(b)
        for _ in range(1, cycles):
            x = x + self.cycle(b - self.As[0] @ x)
        return x

    def pcg(self, A_apply, b, rtol, max_iter):
        """CG of src/cg.hpp:147-222 with this cycle as the preconditioner (stops on r.z)."""
        x = np.zeros_like(b)
        r = b - A_apply(x)
        p = self.cycle(r)
        rz0 = rz = p @ r
        its = 0
        while its < max_iter:
            its += 1
            y = A_apply(p)
            alpha = rz / (p @ y)
            x += alpha * p
            r -= alpha * y
            z = self.cycle(r)
            rz_new = r @ z
            beta = rz_new / rz
            rz = rz_new
            if rz / rz0 < rtol * rtol:
                break
            p = beta * p + z
        return x, its


# ---- the set-up restated ----------------------------------------------------------------------
# Written from the algorithm as the header of csrc/amg_setup.hpp states it (smoothed aggregation: strength
# graph |a_ij| >= theta sqrt(a_ii a_jj), greedy aggregation in three passes, piecewise-constant
# tentative prolongator normalised by 1 / sqrt(size), P = (I - 4 / (3 rho) D^-1 A) T, Galerkin
# product, rho = 1.05 x 20 steps of the power method on D^-1 A), in plain numpy/scipy.  The tests
# compare what the library exports with these functions level by level.

ROW_BLOCK = 4096  # the library adds its norms in blocks of this many rows


class Mt19937_64:
    """The 64-bit Mersenne twister (Matsumoto & Nishimura 2004) = ``std::mt19937_64``."""

    NN, MM = 312, 156
    MASK = (1 << 64) - 1

    def __init__(self, seed):
        mt = [seed & self.MASK]
        for i in range(1, self.NN):
            mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & self.MASK)
        self.mt, self.i = mt, self.NN

    def _twist(self):
        mt, NN, MM = self.mt, self.NN, self.MM
        for i in range(NN):
            x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % NN] & 0x7FFFFFFF)
            mt[i] = mt[(i + MM) % NN] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        self.i = 0

    def __call__(self):
        if self.i >= self.NN:
            self._twist()
        x = self.mt[self.i]
        self.i += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        return x


def mt_uniform_half_one(count, seed=12345):
    """``count`` draws of ``std::uniform_real_distribution<double>(0.5, 1.0)`` from ``std::mt19937_64(seed)`` as
    libstdc++ evaluates them: one 64-bit draw x each, u = double(x) * 2^-64 (the next double below 1 where that rounds
    to 1), value = 0.5 u + 0.5."""
    gen = Mt19937_64(seed)
    out = np.empty(count)
    for i in range(count):
        u = float(gen()) * 2.0 ** -64
        if u >= 1.0:
            u = float(np.nextafter(1.0, 0.0))
        out[i] = 0.5 * u + 0.5
    return out


def hashed_start(global_index):
    """Start vector of the power method on the partitioned operator: a 64-bit mix of the global dof number."""
    with np.errstate(over="ignore"):
        h = np.asarray(global_index).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        h = (h ^ (h >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return 0.5 + 0.5 * (h >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def _block_sum(v):
    """Sum of squares as the library adds it: row blocks one after the other, each added in row order."""
    s = 0.0
    for r0 in range(0, v.size, ROW_BLOCK):
        s += float(np.cumsum(np.square(v[r0:r0 + ROW_BLOCK]))[-1])
    return s


def power_bound(A, its=20, x0=None):
    """Largest eigenvalue of D^-1 A after ``its`` steps of the power method: |D^-1 A x| / |x|, x normalised after
    every step.  ``x0`` None: the library's single-rank start vector (``mt_uniform_half_one``)."""
    n = A.shape[0]
    if n == 0:
        return 1.0
    d = A.diagonal()
    x = mt_uniform_half_one(n) if x0 is None else np.array(x0, dtype=np.float64)
    lam = 1.0
    for _ in range(its):
        y = (A @ x) / d
        nrm = np.sqrt(_block_sum(y))
        if not nrm > 0:
            return 1.0
        lam = nrm / np.sqrt(_block_sum(x))
        x = y / nrm
    return float(lam)


def aggregate(A, theta, stats=None):
    """Greedy aggregation of the CSR matrix ``A`` on its strength graph.  Returns ``(agg, na)``: agg[i] the aggregate
    of row i, -1 = outside the coarse space (no strong coupling).  ``stats`` (a dict), when given, receives the number
    of roots of each pass and of rows outside.

    j is strongly coupled to i when j != i, a_ij != 0 and |a_ij| >= theta sqrt(|a_ii a_jj|) -- one product, one square
    root, one product, so the decision is the library's in IEEE arithmetic."""
    A = A.tocsr()
    n = A.shape[0]
    d = A.diagonal()
    rp, ci, v = A.indptr, A.indices, A.data
    row = np.repeat(np.arange(n), np.diff(rp))
    strong = (ci != row) & (v != 0.0) & (np.abs(v) >= theta * np.sqrt(np.abs(d[row] * d[ci])))
    nbrs = [[] for _ in range(n)]
    wts = [[] for _ in range(n)]
    for i, j, w in zip(row[strong].tolist(), ci[strong].tolist(), np.abs(v[strong]).tolist()):
        nbrs[i].append(j)
        wts[i].append(w)
    FREE = -2
    agg = [FREE if nbrs[i] else -1 for i in range(n)]
    na = 0
    # pass 1: in row order, a row whose whole strong neighbourhood is free becomes a root and takes it
    for i in range(n):
        if agg[i] == FREE and all(agg[j] == FREE for j in nbrs[i]):
            agg[i] = na
            for j in nbrs[i]:
                agg[j] = na
            na += 1
    roots1 = na
    # pass 2: a leftover joins the pass-1 aggregate of its strictly strongest neighbour (the first one wins a tie)
    after1 = list(agg)
    for i in range(n):
        if agg[i] != FREE:
            continue
        best, to = 0.0, FREE
        for j, w in zip(nbrs[i], wts[i]):
            if after1[j] >= 0 and w > best:
                best, to = w, after1[j]
        if to >= 0:
            agg[i] = to
    # pass 3: what is still free forms aggregates of its own, with its free strong neighbours
    for i in range(n):
        if agg[i] != FREE:
            continue
        agg[i] = na
        for j in nbrs[i]:
            if agg[j] == FREE:
                agg[j] = na
        na += 1
    agg = np.array(agg, dtype=np.int64)
    if stats is not None:
        stats.update(pass1_roots=roots1, pass3_roots=na - roots1, outside=int((agg < 0).sum()))
    return agg, na


def smoothed_prolongator(A, agg, na, rho):
    """P = (I - omega D^-1 A) T with omega = 4 / (3 rho) and T[i, agg[i]] = 1 / sqrt(size of the aggregate); rows
    outside the coarse space (agg < 0) are empty, and they contribute nothing to their neighbours' rows."""
    import scipy.sparse as sp

    n = A.shape[0]
    inside = agg >= 0
    size = np.bincount(agg[inside], minlength=na)
    rows = np.nonzero(inside)[0]
    T = sp.csr_matrix((1.0 / np.sqrt(size[agg[rows]].astype(np.float64)), (rows, agg[rows])), shape=(n, na))
    omega = 4.0 / (3.0 * rho)
    P = T - sp.diags(omega / A.diagonal()) @ (A @ T)
    return (sp.diags(inside.astype(np.float64)) @ P).tocsr()


def build(A0, theta0=0.08, coarsest_max=800, max_levels=12):
    """The whole hierarchy from ``A0``: ``(As, Ps, rhos, stats)`` with rho_l = 1.05 power_bound(A_l), theta halved
    from level to level, A_{l+1} = P_l^T A_l P_l.  It stops as the library does: at a level of at most
    ``coarsest_max`` rows, at ``max_levels`` levels, or where aggregation coarsens nothing."""
    As, Ps, rhos, stats = [A0.tocsr()], [], [], []
    theta = theta0
    while True:
        A = As[-1]
        assert A.diagonal().min() > 0.0
        rhos.append(1.05 * power_bound(A))
        if A.shape[0] <= coarsest_max or len(As) >= max_levels:
            break
        st = {}
        agg, na = aggregate(A, theta, st)
        if na == 0 or na >= A.shape[0]:
            break
        P = smoothed_prolongator(A, agg, na, rhos[-1])
        stats.append(st)
        Ps.append(P)
        As.append((P.T @ (A @ P)).tocsr())
        theta *= 0.5
    return As, Ps, rhos, stats
