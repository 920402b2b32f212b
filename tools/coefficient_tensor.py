"""The per-cell diffusion tensor (pmg_laplacian_set_coefficient_tensor) in one process: on the p = orders hierarchy of
n^3 cells, the time of one set_coefficient_tensor on the fine level beside one operator application; the application
and its stiffness kernel (time_kernel) with and without a tensor on the same operator, in the stored and in the affine
geometry mode (the same kernels on the same bytes: expected equal); and the iteration counts of CG preconditioned by
the V-cycle with and without (coarsest level smoothed only, and solved by one AMG cycle).  Prints plain lines; no
threshold.

usage: python tools/coefficient_tensor.py [--n 64] [--orders 1,2,4] [--reps 50] [--rounds 5]

Timing (measuring-on-mi355x): warm-up first; the two versions are compared in the same process, alternating -- every
round sets the tensor, times, removes it, times -- with `reps` back-to-back calls bracketed by HIP events per
timing; the median over the rounds is reported with the smallest and largest round, which is the spread a difference
has to exceed.  set_coefficient_tensor synchronises its stream, so it is timed as wall time around one call with the
device synchronised (it rebuilds the tensor, the per-cell affine tensor and the inverse diagonal)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402


def rotating_tensor(c):
    """Eigenvalues (1, 2 + x, 4), rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre: [ncells, 6] as
    (xx, xy, xz, yy, yz, zz) -- the drivers' --kappa-tensor."""
    n = c.shape[0]
    az, ax = 0.6 + 0.8 * c[:, 1], 0.4 + 0.5 * c[:, 2]
    Rz, Rx = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(az), -np.sin(az), np.sin(az), np.cos(az), 1.0
    Rx[:, 0, 0], Rx[:, 1, 1], Rx[:, 1, 2], Rx[:, 2, 1], Rx[:, 2, 2] = 1.0, np.cos(ax), -np.sin(ax), np.sin(ax), np.cos(ax)
    R = Rz @ Rx
    lam = np.stack([np.ones(n), 2.0 + c[:, 0], np.full(n, 4.0)], axis=1)
    M = np.einsum("nij,nj,nkj->nik", R, lam, R)
    return np.ascontiguousarray(np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1))


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


def pcg_iterations(h, amg=False):
    coarse = pm.AmgSolver(h.operators[0], cycles=1) if amg else None
    h.mg.set_coarse_solver(coarse)
    try:
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(100)
        cg.set_tolerance(1e-8)
        x = h.new_vector()
        x.set(0.0)
        return cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
    finally:
        h.mg.set_coarse_solver(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", default="1,2,4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    orders = tuple(int(t) for t in a.orders.split(","))
    torch.cuda.set_device(0)
    print(f"coefficient_tensor: {torch.cuda.get_device_name(0)}, n = {a.n}, orders = {orders}, K: eigenvalues "
          f"(1, 2 + x, 4) rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) per cell")

    h = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3)
    op, layout = h.operators[-1], h.layouts[-1]
    x, y = h.new_vector(), h.new_vector()
    x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device=x.data.device,
                             generator=torch.Generator(device=x.data.device).manual_seed(0)))
    its_plain = pcg_iterations(h), pcg_iterations(h, amg=True)
    T = torch.from_numpy(rotating_tensor(h.part.xgeom[h.part.geom_dofmap].mean(axis=1))).cuda()
    op.set_coefficient_tensor(T)  # first call: allocates the operator's copy
    set_ms = wall(lambda: op.set_coefficient_tensor(T), a.rounds)
    op.set_coefficient_tensor(None)
    print(f"fine level: degree {orders[-1]}, {layout.size_local} dofs, {op.ncells} cells, "
          f"{op.launches_per_apply()} launches per apply")
    assert op.is_affine()
    for mode in ("stored", "affine"):
        op.set_geometry_mode(mode)
        for _ in range(3):  # warm-up of this mode's kernels, with and without
            op(x, y)
        t = {(w, k): [] for w in (False, True) for k in ("apply", "kernel")}
        for _ in range(a.rounds):
            for with_tensor in (True, False):
                op.set_coefficient_tensor(T if with_tensor else None)
                op(x, y)
                t[with_tensor, "apply"].append(events(lambda: op(x, y), a.reps))
                t[with_tensor, "kernel"].append(op.time_kernel(x, y, a.reps))
        for k, what in (("apply", "apply (HIP events around the whole application)"),
                        ("kernel", "time_kernel (mean of one stiffness launch)")):
            print(f"{mode} mode, {what}: without a tensor {spread(t[False, k])}, with the tensor "
                  f"{spread(t[True, k])}, ratio of the medians "
                  f"{statistics.median(t[True, k]) / statistics.median(t[False, k]):.4f}")
        if mode == "stored":
            print(f"set_coefficient_tensor (tensor, affine tensor and inverse diagonal rebuilt): {set_ms:.3f} ms = "
                  f"{set_ms / statistics.median(t[False, 'apply']):.2f} applies")
    op.set_geometry_mode("stored")
    del h, op, x, y
    ht = pm.PoissonHierarchy(a.n, orders, kappa=2.0, cheb_its=3, kappa_tensor=rotating_tensor)
    its_tensor = pcg_iterations(ht), pcg_iterations(ht, amg=True)
    for i, coarse in enumerate(("coarsest level smoothed only", "coarsest level: one AMG cycle")):
        print(f"PCG (V-cycle preconditioner, rtol 1e-8, {coarse}) iterations without a tensor: {its_plain[i]}, "
              f"with the tensor: {its_tensor[i]}")


if __name__ == "__main__":
    main()
