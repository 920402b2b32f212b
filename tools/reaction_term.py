"""The reaction term (pmg_laplacian_set_reaction) in one process: on the p = orders hierarchy of n^3 cells, the fine
level's operator application and its stiffness kernel (time_kernel, per launch) with and without the term on the same
operator, the time of one set_reaction beside one application, and CG preconditioned by the V-cycle (coarsest level:
one AMG cycle) with and without: iterations and time.  Prints plain lines; no threshold.

usage: python tools/reaction_term.py [--n 64] [--orders 1,2,4] [--reps 50] [--rounds 5] [--plain-only]

--plain-only times the "without" column alone and calls nothing of the reaction term, so the same script runs on a
build of the library from before the term existed: that is how the parent commit's apply is timed in the same
session (profiles/reaction_term.txt).

Timing (measuring-on-mi355x): warm-up first; the two versions are compared in the same process, alternating -- every
round sets the term, times, removes it, times -- with `reps` back-to-back calls bracketed by HIP events per timing;
the median over the rounds is reported with the smallest and largest round, which is the spread a difference has to
exceed.  set_reaction synchronises its stream, so it is timed as wall time around one call with the device
synchronised (it rebuilds the vector and the inverse diagonal)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402

S = 3.0


def linear_sigma(c):
    """sigma_c = S (1 + x_c) at the cell centre -- the drivers' --reaction S."""
    return S * (1.0 + np.asarray(c)[:, 0])


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn, repeats):
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(runs)


def spread(v):
    return f"{statistics.median(v):.4f} ms (rounds {min(v):.4f} .. {max(v):.4f})"


def pcg(h, rounds):
    """(iterations, median wall ms) of PCG to rtol 1e-8 with the V-cycle over one AMG cycle on the coarsest level."""
    h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], cycles=1))
    try:
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(100)
        cg.set_tolerance(1e-8)
        x = h.new_vector()
        its = []

        def solve():
            x.set(0.0)
            its.append(cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg))

        solve()  # warm-up
        return its[0], wall(solve, rounds)
    finally:
        h.mg.set_coarse_solver(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", default="1,2,4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    orders = tuple(int(t) for t in a.orders.split(","))
    torch.cuda.set_device(0)
    print(f"reaction_term: {torch.cuda.get_device_name(0)}, n = {a.n}, orders = {orders}, sigma_c = {S} (1 + x_c) per "
          f"cell{' -- the without column only' if a.plain_only else ''}")

    h = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3)
    op, layout = h.operators[-1], h.layouts[-1]
    x, y = h.new_vector(), h.new_vector()
    x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device=x.data.device,
                             generator=torch.Generator(device=x.data.device).manual_seed(0)))
    print(f"fine level: degree {orders[-1]}, {layout.size_local} dofs, {op.ncells} cells, "
          f"{op.launches_per_apply()} launches per apply")
    versions = (False,) if a.plain_only else (True, False)
    sigma, set_ms = None, None
    if not a.plain_only:
        sigma = torch.from_numpy(linear_sigma(h.part.xgeom[h.part.geom_dofmap].mean(axis=1))).cuda()
        op.set_reaction(sigma)  # first call: allocates the vector
        set_ms = wall(lambda: op.set_reaction(sigma), a.rounds)
        op.set_reaction(None)
    for _ in range(3):  # warm-up
        op(x, y)
    t = {(w, k): [] for w in (False, True) for k in ("apply", "kernel")}
    for _ in range(a.rounds):
        for with_term in versions:
            if not a.plain_only:
                op.set_reaction(sigma if with_term else None)
            op(x, y)
            t[with_term, "apply"].append(events(lambda: op(x, y), a.reps))
            t[with_term, "kernel"].append(op.time_kernel(x, y, a.reps))
    for k, what in (("apply", "apply (HIP events around the whole application)"),
                    ("kernel", "time_kernel (mean of one stiffness launch)")):
        line = f"p = {orders[-1]} {what}: without the term {spread(t[False, k])}"
        if not a.plain_only:
            line += (f", with the term {spread(t[True, k])}, ratio of the medians "
                     f"{statistics.median(t[True, k]) / statistics.median(t[False, k]):.4f}")
        print(line)
    if not a.plain_only:
        print(f"set_reaction (vector and inverse diagonal rebuilt): {set_ms:.3f} ms = "
              f"{set_ms / statistics.median(t[False, 'apply']):.2f} applies")
        op.set_reaction(None)
    its, ms = pcg(h, a.rounds)
    print(f"PCG (V-cycle preconditioner over one AMG cycle, rtol 1e-8) without the term: {its} iterations, {ms:.2f} ms")
    del h, op, x, y
    if not a.plain_only:
        hr = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, reaction=linear_sigma)
        its, ms = pcg(hr, a.rounds)
        print(f"PCG (V-cycle preconditioner over one AMG cycle, rtol 1e-8) with the term: {its} iterations, "
              f"{ms:.2f} ms")


if __name__ == "__main__":
    main()
