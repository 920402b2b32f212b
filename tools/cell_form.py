"""The per-cell bilinear form (pmg_laplacian_cell_form) beside one operator application, in one process, on n^3 cells:

  - the trilinear box, the box bent into a degree-G coordinate element (--curved G), and the box with a per-cell
    coefficient tensor: milliseconds of one cell_form call (kappa, constrained) and of one pmg_laplacian_apply of the
    same operator, and their ratio;
  - the kernel's registers and LDS at the degree, from the compiler's remarks (tools/kernel_resources.py);
  - with --write, the lines appended to profiles/cell_form.md under a heading that names the run.

usage: python tools/cell_form.py [--n 64] [--degree 4 | --degree 1,2,8] [--curved 2] [--reps 20] [--rounds 5] [--write]

Timing (measuring-on-mi355x): warm-up first; the two calls alternate within every round, `reps` back-to-back calls
bracketed by HIP events per timing; the median over the rounds is reported with the smallest and largest round, which is
the spread a difference has to exceed.  No threshold: nobody has measured this kernel before."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import kernel_resources  # noqa: E402


def bend(x):
    return np.stack([x[:, 0] + 0.05 * np.sin(2.0 * x[:, 1] + x[:, 2]), x[:, 1] + 0.05 * np.sin(2.0 * x[:, 2] + x[:, 0]),
                     x[:, 2] + 0.05 * np.sin(2.0 * x[:, 0] + x[:, 1])], axis=1)


def rotating_tensor(c):
    """The drivers' tensor: eigenvalues (1, 2 + x, 4), rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre."""
    n = c.shape[0]
    az, ax = 0.6 + 0.8 * c[:, 1], 0.4 + 0.5 * c[:, 2]
    Rz, Rx = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(az), -np.sin(az), np.sin(az), np.cos(az), 1.0
    Rx[:, 0, 0], Rx[:, 1, 1], Rx[:, 1, 2], Rx[:, 2, 1], Rx[:, 2, 2] = 1.0, np.cos(ax), -np.sin(ax), np.sin(ax), np.cos(ax)
    R = Rz @ Rx
    M = np.einsum("nij,nj,nkj->nik", R, np.stack([np.ones(n), 2.0 + c[:, 0], np.full(n, 4.0)], axis=1), R)
    return np.ascontiguousarray(np.stack([M[:, i, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1))


def resources(degrees):
    rows = kernel_resources.resource_rows("cell_form.hip")
    lines = [kernel_resources.HEADER]
    for P in degrees:
        for name, r in rows.items():
            if re.search(rf"cell_form_kernelILi{P + 1}E", name):
                lines.append(kernel_resources.table_row(f"cell_form_kernel<{P + 1}> (degree {P})", r))
    return lines


def events(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return f"{statistics.median(v):.4f} ms (rounds {min(v):.4f} .. {max(v):.4f})"


def measure(a, P, lines):
    import torch

    import pmg_dolfinx_amd as pm

    cases = (("trilinear box", None, 1, False), (f"box, --curved {a.curved}", bend, a.curved, False),
             ("box with a coefficient tensor", None, 1, True))
    for label, warp, g, tensor in cases:
        part = pm.BoxPartition(a.n, warp=warp, geom_degree=g)
        lv = part.level(P)
        layout = pm.make_layout(lv)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout, geometry_degree=g)
        if tensor:
            m = g + 1
            corners = [((i * g) * m + j * g) * m + k * g for i in (0, 1) for j in (0, 1) for k in (0, 1)]
            op.set_coefficient_tensor(rotating_tensor(part.xgeom[part.geom_dofmap[:, corners]].mean(axis=1)))
        x, y = pm.Vector(layout), pm.Vector(layout)
        x.data.copy_(torch.randn(x.data.numel(), dtype=torch.float64, device="cuda",
                                 generator=torch.Generator(device="cuda").manual_seed(0)))
        out = torch.empty(part.ncells, dtype=torch.float64, device="cuda")
        form = lambda: op.cell_form(x, x, out=out, kappa=True, constrained=True)  # noqa: E731
        apply = lambda: op(x, y)  # noqa: E731
        for _ in range(3):
            form()
            apply()
        t = {"form": [], "apply": []}
        for _ in range(a.rounds):
            t["form"].append(events(torch, form, a.reps))
            t["apply"].append(events(torch, apply, a.reps))
        ratio = statistics.median(t["form"]) / statistics.median(t["apply"])
        # the identity of the driver's --cell-form, as a check that the timed call computed something
        m_ = torch.from_numpy(lv.bc_marker.astype(bool)).cuda()
        xm = torch.where(m_, torch.zeros_like(x.data), x.data)
        energy, dot = float(out.sum()), float(xm @ y.data)
        lines.append(f"degree {P}, {a.n}^3 cells, {label}: cell_form {spread(t['form'])}, apply {spread(t['apply'])}, "
                     f"ratio of the medians {ratio:.3f}; sum_c e_c = {energy:.15e}, u_m . y = {dot:.15e}, "
                     f"relative difference {abs(energy - dot) / abs(dot):.2e}")
        print(lines[-1], flush=True)
        del op, x, y, out, layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--degree", default="4")
    ap.add_argument("--curved", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/cell_form.md")
    ap.add_argument("--resources-only", action="store_true", help="the compiler's table only (no GPU needed)")
    a = ap.parse_args()
    degrees = [int(p) for p in a.degree.split(",")]
    lines = []
    if not a.resources_only:
        import torch

        torch.cuda.set_device(0)
        lines.append(f"Device: {torch.cuda.get_device_name(0)}; reps {a.reps}, rounds {a.rounds}.")
        print(lines[-1])
        for P in degrees:
            measure(a, P, lines)
    table = resources(degrees)
    print("\n".join(table))
    if a.write:
        path = os.path.join(ROOT, "profiles", "cell_form.md")
        with open(path, "a") as f:
            f.write(f"\n## Run: `python tools/cell_form.py {' '.join(sys.argv[1:])}`\n\n")
            f.write("".join(f"- {l}\n" for l in lines) + "\n" + "\n".join(table) + "\n")
        print("appended to", path)


if __name__ == "__main__":
    main()
