"""FP64 against FP32 in one process: the stiffness apply per degree, the V-cycle (plain and with the AMG coarse
solver) and PCG to 1e-8 (iterations and wall time), on the same hierarchy, both precisions timed the same way.
Prints one JSON line.

usage: python tools/fp32_cycle.py [--n 64] [--orders 1,2,4] [--orders 1,3,6] [--reps 20] [--repeats 5] [--cheb-its 3]

Timing (measuring-on-mi355x): warm-up first, then `repeats` timed runs of `reps` back-to-back calls bracketed by
HIP events; the median run is reported.  The FP32 kernel's fraction of 8 TB/s is computed on the byte model
24N [float G] + 4N [patch lists] + 9U [x, y, bc] bytes per cell (kappa: 12 B per cell, left out), next to the FP64 model
48N + 4N + 8 + 17U (bench.py)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402

HBM_PEAK_GBS = 8000.0


def bytes_fp64(P):
    N, U = (P + 1) ** 3, P**3
    return 48 * N + 4 * N + 8 + 17 * U


def bytes_fp32(P):
    N, U = (P + 1) ** 3, P**3
    return 24 * N + 4 * N + 9 * U


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


def pcg(h, rtol):
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(100)
    cg.set_tolerance(rtol)
    x = h.new_vector()
    x.set(0.0)
    cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)  # warm-up (graphs, float tensors)
    x.set(0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    r = pm.Vector(h.layouts[-1])
    h.operators[-1](x, r)
    pm.axpy(r, -1.0, r, h.rhs[-1])
    return its, wall, pm.norm(r) / pm.norm(h.rhs[-1])


def one_config(n, orders, reps, repeats, cheb_its=3):
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=cheb_its)
    out = {"n": n, "orders": list(orders), "cheb_its": cheb_its, "fine_dofs": h.fine_ndofs_owned, "apply": {}}
    for P, op, lay in zip(orders, h.operators, h.layouts):
        ncells = h.part.ncells
        x64, y64 = pm.Vector(lay), pm.Vector(lay)
        x64.set(1.0)
        x32 = torch.ones(lay.size_local + lay.num_ghosts, dtype=torch.float32, device="cuda")
        y32 = torch.empty_like(x32)
        ms64 = timed(lambda: op(x64, y64), reps, repeats)
        ms32 = timed(lambda: op.apply_fp32(x32, y32), reps, repeats)
        out["apply"][f"p{P}"] = {
            "fp64_ms": round(ms64, 4), "fp32_ms": round(ms32, 4), "ratio": round(ms32 / ms64, 3),
            "fp64_frac_8TBs": round(bytes_fp64(P) * ncells / (ms64 * 1e-3) / 1e9 / HBM_PEAK_GBS, 3),
            "fp32_frac_8TBs": round(bytes_fp32(P) * ncells / (ms32 * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)}
    b = h.rhs[-1]
    x = h.new_vector()
    for coarse in ("plain", "amg"):
        h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], cycles=2) if coarse == "amg" else None)
        row = {}
        for prec in ("fp64", "fp32"):
            h.mg.set_precision(prec)
            x.set(0.0)
            row[f"{prec}_ms"] = round(timed(lambda: h.mg.apply(b, x), reps, repeats), 4)
        row["ratio"] = round(row["fp32_ms"] / row["fp64_ms"], 3)
        out[f"cycle_{coarse}"] = row
    row = {}
    for prec in ("fp64", "fp32"):  # stationary AMG coarse solver: a fixed linear preconditioner, plain CG
        h.mg.set_precision(prec)
        its, wall, res = pcg(h, 1e-8)
        row[prec] = {"iterations": its, "wall_ms": round(wall, 2), "true_rel_residual": float(f"{res:.3e}")}
    row["wall_ratio"] = round(row["fp32"]["wall_ms"] / row["fp64"]["wall_ms"], 3)
    out["pcg_amg_1e-8"] = row
    h.mg.set_precision("fp64")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", action="append", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cheb-its", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    configs = [tuple(int(p) for p in o.split(",")) for o in (a.orders or ["1,2,4"])]
    res = {"tool": "fp32_cycle", "device": torch.cuda.get_device_name(0),
           "configs": [one_config(a.n, o, a.reps, a.repeats, a.cheb_its) for o in configs]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
