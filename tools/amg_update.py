"""pmg_amg_update_values against pmg_amg_create on one GPU (profiles/amg_update.md).

    python tools/amg_update.py --n 64

For each mesh size: create and update timed whole, three runs each, alternating (the update after a change of the
per-cell tensor, so it has work to do; the first update, which plans on the host, timed apart); the stage laps of
both with PMG_AMG_TIMING set (written to stderr by the library); device bytes in use before and after the first
update; the largest relative difference of a renewed bound from numpy's power method on the exported matrix; and the
iterations of the AMG-preconditioned CG on the degree-1 operator (rtol 1e-8, random right-hand side) with a fresh, a
renewed and the stale hierarchy, for the drivers' --kappa-field and --kappa-tensor coefficients."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 32])
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    import pmg_dolfinx_amd as pm
    import tensor_coefficient_reference as tr
    from oracle import amg_oracle as ao

    torch.cuda.set_device(0)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free

    for n in args.n:
        part = pm.BoxPartition(n)
        lv = part.level(1)
        layout = pm.make_layout(lv)
        op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
        op.compute_diag_inverse()
        centres = tr.cell_centres(part.xgeom, part.geom_dofmap)
        c = part.dof_coordinates(1)
        T = tr.rotating_tensor(centres)
        kq = pm.Vector(layout)
        kq.data.copy_(torch.from_numpy(1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1]) + c[:, 2]))
        b = np.random.default_rng(5).standard_normal(lv.ndofs)
        b[lv.bc_marker.astype(bool)] = 0.0
        bv, x = pm.Vector(layout), pm.Vector(layout)
        bv.data.copy_(torch.from_numpy(b))

        print(f"== {n}^3 cells, {lv.ndofs} rows ==")
        amg, ms = wall(lambda: pm.AmgSolver(op, max_iter=200, rtol=1e-8))
        print(f"create (first, library warm-up included): {ms:8.1f} ms; levels "
              f"{[(i['rows'], i['nnz']) for i in amg.info()]}")
        before = used()
        _, ms = wall(amg.update_values)
        print(f"first update (plans on the host): {ms:8.1f} ms; device bytes in use {before} -> {used()} "
              f"(+{(used() - before) / 2**20:.1f} MiB); structural {[(i['rows'], i['nnz']) for i in amg.info()]}")
        scale = 1.0
        for r in range(args.runs):
            other, t_create = wall(lambda: pm.AmgSolver(op, max_iter=200, rtol=1e-8))
            del other
            scale *= 1.5
            op.set_coefficient_tensor(np.ascontiguousarray(scale * T))
            _, t_update = wall(amg.update_values)
            print(f"run {r}: create {t_create:8.1f} ms   update {t_update:8.2f} ms   ratio {t_create / t_update:6.1f}")
        op.set_coefficient_tensor(None)
        os.environ["PMG_AMG_TIMING"] = "1"
        sys.stdout.flush()
        print("stage laps, create then update (stderr):", flush=True)
        other = pm.AmgSolver(op)
        del other
        amg.update_values()
        del os.environ["PMG_AMG_TIMING"]
        worst = 0.0
        for l in range(amg.num_levels()):
            want = 1.05 * ao.power_bound(amg.export(l, "A"))
            worst = max(worst, abs(amg.level_info(l)["lambda_max"] - want) / want)
        print(f"largest relative difference of a renewed bound from numpy's: {worst:.2e}")

        for name, setter, value in (("--kappa-field", op.set_coefficient_field, kq),
                                    ("--kappa-tensor", op.set_coefficient_tensor, T)):
            amg.update_values()  # the constant-coefficient hierarchy again
            stale = pm.AmgSolver(op, max_iter=200, rtol=1e-8)
            setter(value)
            op.compute_diag_inverse()
            amg.update_values()
            fresh = pm.AmgSolver(op, max_iter=200, rtol=1e-8)
            its = {k: s.solve(x, bv) for k, s in (("fresh", fresh), ("renewed", amg), ("stale", stale))}
            print(f"{name}: CG iterations to 1e-8: {its}")
            setter(None)
            op.compute_diag_inverse()
            del stale, fresh


if __name__ == "__main__":
    main()
