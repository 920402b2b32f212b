"""Curved cells (pmg_laplacian_create_curved) in one process, on n^3 cells of the quarter annulus at degree p:

  - the milliseconds to build the geometry tensor with the trilinear kernel (g = 1, the baseline), and at g = 2 and
    g = 4 by both paths: the cell-cooperative sum-factorised kernel (the library's own tabulation) and the per-point
    kernel over the dense table (the same tabulation handed back as caller tables);
  - time_kernel of the apply on the curved operator beside the straight one (the same kernel over the same bytes:
    expected equal);
  - one batched-geometry application (the tensor recomputed in every application) at g = 1 and g = 2.

usage: python tools/curved_geometry.py [--n 32] [--degree 4] [--reps 20] [--rounds 5]

Timing (measuring-on-mi355x): warm-up first; everything is compared in one process, the operators alternating within
every round, `reps` back-to-back calls bracketed by HIP events per timing; the median over the rounds is reported with
the smallest and largest round, which is the spread a difference has to exceed.  The build of the tensor is timed as
the export of the tensor (pmg_laplacian_get_geometry) in batched mode with one batch holding every patch -- build, then
export -- minus the export of the resident tensor: the same export kernel over the same bytes, so the difference is
the geometry kernel alone.  Prints plain lines; no threshold."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmg_dolfinx_amd as pm  # noqa: E402
from pmg_dolfinx_amd import _lib, _tables  # noqa: E402


def quarter_annulus(x):
    r, t = 1.0 + x[:, 0], 0.5 * np.pi * x[:, 1]
    return np.stack([r * np.cos(t), r * np.sin(t), x[:, 2]], axis=1)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return f"{statistics.median(v):.4f} ms (rounds {min(v):.4f} .. {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    P, N = a.degree, (a.degree + 1) ** 3
    torch.cuda.set_device(0)
    print(f"curved_geometry: {torch.cuda.get_device_name(0)}, {a.n}^3 cells of the quarter annulus, degree {P}")

    ops = {}
    layout = None
    for g, path in ((1, "trilinear"), (2, "cooperative"), (2, "per-point"), (4, "cooperative"), (4, "per-point")):
        part = pm.BoxPartition(a.n, warp=quarter_annulus, geom_degree=g)
        lv = part.level(P)
        layout = layout or pm.make_layout(lv)
        kw = {}
        if path == "per-point":
            kw = dict(dphi_geometry=pm.coordinate_element_table(P, g), G_weights=np.einsum(
                "a,b,c->abc", *([_tables.gll_points_weights(P + 1)[1]] * 3)).ravel())
        ops[g, path] = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                           lv.bc_marker, layout, geometry_degree=g, **kw)
    ncells = a.n**3
    out = torch.empty((ncells, N, 6), dtype=torch.float64, device="cuda")
    x, y = pm.Vector(layout), pm.Vector(layout)
    x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device="cuda",
                             generator=torch.Generator(device="cuda").manual_seed(0)))

    def export(op):
        _lib.call("pmg_laplacian_get_geometry", op.handle, _lib.ptr(out), _lib.current_stream())

    build = {k: [] for k in ops}
    for rnd in range(a.rounds + 1):  # (round 0: warm-up)
        for k, op in ops.items():
            export(op)
            resident = events(lambda: export(op), a.reps)
            _lib.call("pmg_laplacian_set_geometry_batch", op.handle, ncells)
            export(op)
            batched = events(lambda: export(op), a.reps)
            _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)
            if rnd:
                build[k].append(batched - resident)
    base = statistics.median(build[1, "trilinear"])
    for k, v in build.items():
        print(f"tensor build, g = {k[0]}, {k[1]} kernel: {spread(v)}, {statistics.median(v) / base:.2f} x the "
              f"trilinear kernel, {1e-6 * ncells * N / statistics.median(v):.1f} Gpoints/s")

    straight, curved = ops[1, "trilinear"], ops[2, "cooperative"]
    for op in (straight, curved):
        for _ in range(3):
            op(x, y)
    t = {"straight": [], "curved": []}
    for _ in range(a.rounds):
        t["straight"].append(straight.time_kernel(x, y, a.reps))
        t["curved"].append(curved.time_kernel(x, y, a.reps))
    print(f"time_kernel of the apply: straight (g = 1) {spread(t['straight'])}, curved (g = 2) {spread(t['curved'])}, "
          f"ratio of the medians {statistics.median(t['curved']) / statistics.median(t['straight']):.4f}")

    t = {"resident": {1: [], 2: []}, "batched": {1: [], 2: []}}
    for mode, cells in (("resident", 0), ("batched", max(ncells // 4, 1))):
        for g, op in ((1, straight), (2, curved)):
            _lib.call("pmg_laplacian_set_geometry_batch", op.handle, cells)
            op(x, y)
        for _ in range(a.rounds):
            for g, op in ((1, straight), (2, curved)):
                t[mode][g].append(events(lambda: op(x, y), a.reps))
        for g, op in ((1, straight), (2, curved)):
            _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)
    for mode in ("resident", "batched"):
        print(f"one application, {mode} geometry"
              + (f" (batches of {max(ncells // 4, 1)} cells)" if mode == "batched" else "")
              + f": g = 1 {spread(t[mode][1])}, g = 2 {spread(t[mode][2])}")


if __name__ == "__main__":
    main()
