"""The assembled CSR operator against the matrix-free one, in one process: per degree 1 ... 4 the set-up time split
into pattern (host) and values (device), the bytes held, SpMV against the matrix-free apply on the same vector; then
the p = 4 -> 2 -> 1 V-cycle with level 0 assembled against the all-matrix-free cycle.  Prints one JSON line.

usage: python tools/matrix_operator.py [--n 24] [--reps 20] [--repeats 5]

n = 24 (or 32) keeps the degree-4 matrix on the card: (P + 2)^3 entries per row on average, 12 bytes each.
Timing (measuring-on-mi355x): warm-up first, then `repeats` timed runs of `reps` back-to-back calls bracketed by HIP
events; the median run is reported.  Set-up is wall time around one call, device synchronised: values = one
update_values() on the existing pattern, pattern = the constructor minus that."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def one_degree(n, P, reps, repeats):
    part = pm.BoxPartition(n)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker, layout)
    M, create_ms = wall(lambda: pm.MatrixOperator(op))
    _, values_ms = wall(M.update_values)
    x, y = pm.Vector(layout), pm.Vector(layout)
    x.set(1.0)
    spmv = timed(lambda: M(x, y), reps, repeats)
    free = timed(lambda: op(x, y), reps, repeats)
    return {"degree": P, "rows": M.rows, "nnz": M.nnz, "mean_row": round(M.nnz / M.rows, 1),
            "setup_pattern_ms": round(create_ms - values_ms, 1), "setup_values_ms": round(values_ms, 2),
            "matrix_bytes": M.nbytes, "csr_bytes_per_row": round(12.0 * M.nnz / M.rows, 1),
            "spmv_ms": round(spmv, 4), "matfree_ms": round(free, 4), "spmv_over_matfree": round(spmv / free, 3)}


def cycle(n, reps, repeats):
    h = pm.PoissonHierarchy(n, (1, 2, 4), kappa=2.0, cheb_its=3)
    x = h.new_vector()
    x.set(0.0)
    free = timed(lambda: h.mg.apply(h.rhs[-1], x), reps, repeats)
    M = pm.MatrixOperator(h.operators[0])
    h.mg.set_level_matrix(0, M)
    x.set(0.0)
    mixed = timed(lambda: h.mg.apply(h.rhs[-1], x), reps, repeats)
    h.mg.set_level_matrix(0, None)
    return {"orders": [1, 2, 4], "matfree_ms": round(free, 4), "level0_assembled_ms": round(mixed, 4),
            "ratio": round(mixed / free, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"tool": "matrix_operator", "device": torch.cuda.get_device_name(0), "n": a.n,
           "degrees": [one_degree(a.n, P, a.reps, a.repeats) for P in (1, 2, 3, 4)],
           "cycle": cycle(a.n, a.reps, a.repeats)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
