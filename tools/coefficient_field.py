"""The nodal coefficient field (pmg_laplacian_set_coefficient_field) in one process: on the p = orders hierarchy of
n^3 cells, the time of one set_coefficient_field on the fine level beside one operator application, the application
with and without a field (the same kernels on the same bytes: expected equal), and the iteration counts of CG
preconditioned by the V-cycle with and without (coarsest level smoothed only, and solved by one AMG cycle).  Prints
plain lines; no threshold.

usage: python tools/coefficient_field.py [--n 64] [--orders 1,2,4] [--reps 20] [--repeats 5]

Timing (measuring-on-mi355x): warm-up first, then `repeats` timed runs of `reps` back-to-back calls bracketed by HIP
events; the median run is reported.  set_coefficient_field synchronises its stream, so it is timed as wall time around
one call with the device synchronised, median of `repeats` (it rebuilds the tensor and the inverse diagonal)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402


def smooth_field(c):
    return 1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1]) + c[:, 2]


def timed(fn, reps, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / reps)
    return statistics.median(runs)


def wall(fn, repeats):
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(runs)


def pcg_iterations(h, amg=False):
    """CG on the fine level preconditioned by the V-cycle; amg: the coarsest level solved by one AMG cycle built on
    that level's operator (field included) instead of being smoothed only."""
    coarse = pm.AmgSolver(h.operators[0], cycles=1) if amg else None
    h.mg.set_coarse_solver(coarse)
    try:
        return _pcg(h)
    finally:
        h.mg.set_coarse_solver(None)


def _pcg(h):
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(100)
    cg.set_tolerance(1e-8)
    x = h.new_vector()
    x.set(0.0)
    return cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", default="1,2,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    orders = tuple(int(t) for t in a.orders.split(","))
    torch.cuda.set_device(0)
    print(f"coefficient_field: {torch.cuda.get_device_name(0)}, n = {a.n}, orders = {orders}, "
          f"kq = 1 + 0.5 sin(2 pi x) cos(2 pi y) + z")

    h = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3)
    op, layout = h.operators[-1], h.layouts[-1]
    x, y = h.new_vector(), h.new_vector()
    x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device=x.data.device,
                             generator=torch.Generator(device=x.data.device).manual_seed(0)))
    apply_plain = timed(lambda: op(x, y), a.reps, a.repeats)
    its_plain = pcg_iterations(h), pcg_iterations(h, amg=True)
    kq = pm.Vector(layout)
    kq.data.copy_(torch.from_numpy(smooth_field(h.part.dof_coordinates(orders[-1]))))
    op.set_coefficient_field(kq)  # first call: allocates the operator's copy
    set_ms = wall(lambda: op.set_coefficient_field(kq), a.repeats)
    apply_field = timed(lambda: op(x, y), a.reps, a.repeats)
    op.set_coefficient_field(None)
    apply_again = timed(lambda: op(x, y), a.reps, a.repeats)
    del h, op, x, y, kq
    hf = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, kappa_field=smooth_field)
    its_field = pcg_iterations(hf), pcg_iterations(hf, amg=True)

    print(f"fine level: degree {orders[-1]}, {layout.size_local} dofs")
    print(f"set_coefficient_field (tensor + inverse diagonal rebuilt): {set_ms:.3f} ms = "
          f"{set_ms / apply_plain:.2f} applies")
    print(f"apply without a field: {apply_plain:.4f} ms")
    print(f"apply with the field:  {apply_field:.4f} ms (ratio {apply_field / apply_plain:.4f})")
    print(f"apply, field removed:  {apply_again:.4f} ms (ratio {apply_again / apply_plain:.4f})")
    # (the manufactured load is an eigenfunction of the constant-coefficient operator on the uniform grid, which a
    # smoothed-only coarse level gets away with; with a field it is not, and the coarse solve shows)
    for i, coarse in enumerate(("coarsest level smoothed only", "coarsest level: one AMG cycle")):
        print(f"PCG (V-cycle preconditioner, rtol 1e-8, {coarse}) iterations without a field: {its_plain[i]}, "
              f"with the field: {its_field[i]}")


if __name__ == "__main__":
    main()
