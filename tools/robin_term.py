"""The Robin boundary term (pmg_laplacian_set_robin) in one process: on the p = orders hierarchy of n^3 cells, the
fine level's operator application and its stiffness kernel (time_kernel, per launch) with and without the term on the
same operator, the time of one set_robin beside one application, and CG preconditioned by the V-cycle (coarsest level:
one AMG cycle) with and without: iterations and time.  Prints plain lines; no threshold.

usage: python tools/robin_term.py [--n 64] [--orders 1,2,4] [--reps 50] [--rounds 5] [--plain-only]

The problem is the drivers' --robin A: the Dirichlet marker on the face x = 0 only, alpha = A (1 + y) at the facet
points of the other five faces, on every level.  --plain-only keeps that marker, times the "without" column alone and
calls nothing of the Robin term, so the same script runs on a build of the library from before the term existed: that
is how the parent commit's apply is timed in the same session (profiles/robin_term.txt).

Timing (measuring-on-mi355x): warm-up first; the two versions are compared in the same process, alternating -- every
round sets the term, times, removes it, times -- with `reps` back-to-back calls bracketed by HIP events per timing;
the median over the rounds is reported with the smallest and largest round, which is the spread a difference has to
exceed.  set_robin synchronises its stream, so it is timed as wall time around one call with the device synchronised
(it uploads the facet lists and rebuilds the vector and the inverse diagonal)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402

A = 2.0


def linear_alpha(pts):
    """alpha = A (1 + y) at the facet point -- the drivers' --robin A."""
    return A * (1.0 + np.asarray(pts)[:, 1])


def x0_face(c):
    return np.abs(np.asarray(c)[:, 0]) < 1e-12


def robin_facets(part, P):
    """The facet lists of the five faces other than x = 0 and alpha at their facet points of degree P.  (Written with
    the mesh's dofmap and dof coordinates alone, so that --plain-only needs nothing newer than the parent commit.)"""
    cells, facets = part.exterior_facets()
    keep = facets != 0
    cells, facets = cells[keep], facets[keep]
    nodes = np.stack([pm.facet_nodes(P, f) for f in range(6)])
    pts = part.dof_coordinates(P)[part.level(P).dofmap[cells.astype(np.int64)[:, None], nodes[facets.astype(np.int64)]]]
    return cells, facets, linear_alpha(pts.reshape(-1, 3)).reshape(cells.size, -1)


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
    print(f"robin_term: {torch.cuda.get_device_name(0)}, n = {a.n}, orders = {orders}, Dirichlet on x = 0, alpha = {A} "
          f"(1 + y) on the other five faces{' -- the without column only' if a.plain_only else ''}")

    h = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, dirichlet=x0_face)
    op, layout = h.operators[-1], h.layouts[-1]
    x, y = h.new_vector(), h.new_vector()
    x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device=x.data.device,
                             generator=torch.Generator(device=x.data.device).manual_seed(0)))
    print(f"fine level: degree {orders[-1]}, {layout.size_local} dofs, {op.ncells} cells, "
          f"{op.launches_per_apply()} launches per apply")
    versions = (False,) if a.plain_only else (True, False)
    set_ms = None
    if not a.plain_only:
        cells, facets, alpha = robin_facets(h.part, orders[-1])
        alpha = torch.from_numpy(np.ascontiguousarray(alpha)).cuda()
        print(f"{cells.size} facets, {alpha.numel()} facet points")
        op.set_robin(cells, facets, alpha)  # first call: allocates the vector
        set_ms = wall(lambda: op.set_robin(cells, facets, alpha), a.rounds)
        op.set_robin(None, None, None)
    for _ in range(3):  # warm-up
        op(x, y)
    t = {(w, k): [] for w in (False, True) for k in ("apply", "kernel")}
    for _ in range(a.rounds):
        for with_term in versions:
            if not a.plain_only:
                if with_term:
                    op.set_robin(cells, facets, alpha)
                else:
                    op.set_robin(None, None, None)
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
        print(f"set_robin (lists uploaded, vector and inverse diagonal rebuilt): {set_ms:.3f} ms = "
              f"{set_ms / statistics.median(t[False, 'apply']):.2f} applies")
        op.set_robin(None, None, None)
    its, ms = pcg(h, a.rounds)
    print(f"PCG (V-cycle preconditioner over one AMG cycle, rtol 1e-8) without the term: {its} iterations, {ms:.2f} ms")
    del h, op, x, y
    if not a.plain_only:
        hr = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, dirichlet=x0_face,
                                 robin=lambda pts: np.where(x0_face(pts), 0.0, linear_alpha(pts)))
        its, ms = pcg(hr, a.rounds)
        print(f"PCG (V-cycle preconditioner over one AMG cycle, rtol 1e-8) with the term: {its} iterations, "
              f"{ms:.2f} ms")


if __name__ == "__main__":
    main()
