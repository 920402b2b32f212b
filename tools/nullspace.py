"""The constant null space (pmg_cg_set_nullspace) in one process: on the fine level of the p = orders hierarchy of n^3
cells WITHOUT any Dirichlet dof and with a compatible right-hand side, the time of one PCG iteration with the mode off
and on -- Jacobi, and the V-cycle over a stationary AMG (2 cycles, its own null space set in both columns: only the outer
CG differs) --, the iteration counts to rtol 1e-8, and the drift |1 . x| / |x|_1 of the plain iteration.  Prints plain
lines; no threshold.

usage: python tools/nullspace.py [--n 64] [--orders 1,2,4] [--its 30] [--rounds 5]

Timing (measuring-on-mi355x): warm-up first; the two modes are compared in the same process, alternating round by
round; one timing is the wall time of a solve of exactly `its` iterations (rtol 0) with the device synchronised around
it, divided by `its` (the set-up of a solve -- one application, the first preconditioner call, with the mode on the two
projections -- is spread over the iterations); the median over the rounds is reported with the smallest and largest
round, which is the spread a difference has to exceed.

Launches per iteration are counted from the loop (csrc/solvers.hip), A = launches of one operator application:
  Jacobi, off: A + dot (2) + update + dot (2) + direction            = A + 6
  Jacobi, on:  A + dot (2) + update + three sums (2) + direction     = A + 6
  V-cycle, off / on: the same with the cycle's launches in front of the second reduction."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402


def solve(h, cg, mode, rtol, max_iter, precond):
    cg.set_nullspace(mode)
    cg.set_tolerance(rtol)
    cg.set_max_iterations(max_iter)
    x = h.new_vector()
    x.set(0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    its = cg.solve(h.operators[-1], x, h.b, preconditioner=precond)
    torch.cuda.synchronize()
    return x, its, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", default="1,2,4")
    ap.add_argument("--its", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    orders = tuple(int(v) for v in a.orders.split(","))
    torch.cuda.set_device(0)
    h = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, dirichlet=lambda c: c[:, 0] < -1.0)
    assert all(lv.bc_marker.sum() == 0 for lv in h.levels)
    h.b = h.rhs[-1]
    h.b.remove_mean()
    amg = pm.AmgSolver(h.operators[0], cycles=2)
    amg.set_nullspace("constant")
    h.mg.set_coarse_solver(amg)
    n = h.levels[-1].ndofs
    A = pm._lib.call("pmg_laplacian_launches_per_apply", h.operators[-1].handle)
    print(f"n = {a.n}, orders {orders}: {n} fine dofs, no Dirichlet dof; operator application = {A} launches")
    cg = pm.CGSolver(h.layouts[-1])
    for name, precond in (("Jacobi", None), ("V-cycle + AMG(2)", h.mg)):
        for mode in (None, "constant"):  # warm-up
            solve(h, cg, mode, 0.0, 3, precond)
        per = {None: [], "constant": []}
        cap = a.its if precond is None else min(a.its, 8)  # (the V-cycle PCG reaches rounding level soon after)
        for _ in range(a.rounds):
            for mode in (None, "constant"):
                _, its, ms = solve(h, cg, mode, 0.0, cap, precond)
                assert its == cap, (its, cap)
                per[mode].append(ms / its)
        line = []
        for mode in (None, "constant"):
            v = per[mode]
            line.append(f"{'on ' if mode else 'off'} {statistics.median(v):8.4f} ms/iteration "
                        f"[{min(v):.4f}, {max(v):.4f}]")
        off, on = statistics.median(per[None]), statistics.median(per["constant"])
        print(f"{name:18s} {line[0]};  {line[1]};  on / off = {on / off:.4f}")
        x_off, its_off, _ = solve(h, cg, None, 1e-8, 2000, precond)
        x_on, its_on, _ = solve(h, cg, "constant", 1e-8, 2000, precond)
        xo, xn = x_off.data_copy(), x_on.data_copy()
        print(f"{'':18s} iterations to rtol 1e-8: off {its_off}, on {its_on};  |1 . x| / |x|_1: off "
              f"{abs(xo.sum()) / np.abs(xo).sum():.3e}, on {abs(xn.sum()) / np.abs(xn).sum():.3e}")
        print(f"{'':18s} launches per iteration besides the preconditioner: off {A} + 6, on {A} + 6")


if __name__ == "__main__":
    main()
