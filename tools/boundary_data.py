#!/usr/bin/env python3
"""Cost of the Dirichlet lifting (pmg_laplacian_apply_lifting) beside one operator application, and beside the route
it replaces: a second complete operator with an all-zero marker plus one full-volume application of it
(examples/cg/cg_main.cpp without --lift).

    python tools/boundary_data.py --n 64 --orders 4 [--reps 20] [--out profiles/boundary_data.txt]

Times are HIP-event times on the current stream, the mean of --reps calls after two warm-up calls; the first lifting
call (which reads the dofmap and the marker back and builds the cell list) and the creation of the second operator
are wall-clock times with a device synchronisation on either side.  Device bytes are differences of hipMemGetInfo."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn, reps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--orders", type=int, nargs="+", default=[4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import __graft_entry__ as g

    g.build()
    import pmg_dolfinx_amd as pm
    from pmg_dolfinx_amd import _lib

    torch.cuda.set_device(0)
    lines = [f"boundary data on {torch.cuda.get_device_name(0)}: {a.n}^3 cells, {a.reps} timed calls each"]
    for P in a.orders:
        part = pm.BoxPartition(a.n)
        lv = part.level(P)
        layout = pm.make_layout(lv)
        dev = layout.device
        args = dict(dofmap=torch.from_numpy(lv.dofmap).to(dev), xgeom=torch.from_numpy(part.xgeom).to(dev),
                    gd=torch.from_numpy(part.geom_dofmap).to(dev),
                    kappa=torch.full((part.ncells,), 2.0, dtype=torch.float64, device=dev))

        def make(marker):
            return pm.MatFreeLaplacian(P, args["kappa"], args["dofmap"], args["xgeom"], args["gd"], lv.lcells,
                                       lv.bcells, marker, layout)

        op = make(lv.bc_marker)
        m = lv.bc_marker.astype(bool)
        gv, b, x, y = (pm.Vector(layout) for _ in range(4))
        gv.data.copy_(torch.from_numpy(np.where(m, 1.3, np.nan)))
        b.set(0.0)
        x.set(1.0)
        t_apply = event_ms(lambda: op(x, y), a.reps)
        t_first, _ = wall_s(lambda: op.apply_lifting(gv, b))
        shell = op.lift_cell_count()
        t_lift = event_ms(lambda: op.apply_lifting(gv, b), a.reps)
        t_setbc = event_ms(lambda: op.set_bc(gv, b), a.reps)
        # the route it replaces
        before = used_bytes()
        t_create, op_free = wall_s(lambda: make(np.zeros(lv.ndofs, dtype=np.int8)))
        held = used_bytes() - before
        tensor = _lib.call("pmg_laplacian_geometry_bytes", op_free.handle)
        gm = pm.Vector(layout)
        gm.data.copy_(torch.from_numpy(np.where(m, 1.3, 0.0)))
        t_free = event_ms(lambda: op_free(gm, y), a.reps)
        # the two routes agree
        b.set(0.0)
        op.apply_lifting(gv, b, alpha=-1.0)
        op_free(gm, y)
        torch.cuda.synchronize()
        got, old = b.data_copy()[~m], y.data_copy()[~m]
        agree = np.abs(got - old).max() / np.abs(old).max()
        lines += [
            f"degree {P}: {lv.ndofs} dofs, {part.ncells} cells, {shell} of them hold a Dirichlet dof "
            f"({100.0 * shell / part.ncells:.1f} %)",
            f"  one operator application            {t_apply:10.4f} ms",
            f"  apply_lifting                       {t_lift:10.4f} ms  ({t_lift / t_apply:.3f} of an application)",
            f"  apply_lifting, first call           {t_first * 1e3:10.2f} ms  (wall; reads dofmap and marker back, "
            f"builds the list)",
            f"  set_bc                              {t_setbc:10.4f} ms",
            f"  old route: create a second operator {t_create * 1e3:10.2f} ms  (wall)",
            f"  old route: one application of it    {t_free:10.4f} ms",
            f"  old route holds                     {held / 1e6:10.1f} MB of device memory "
            f"(geometry tensor {tensor / 1e6:.1f} MB)",
            f"  lifting vs old route, unmarked rows {agree:10.2e}  (max|a-b| / max|b|)",
        ]
        del op_free, op
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
