"""The coefficient gradients of the form (pmg_laplacian_form_gradients) beside the cell form and one operator
application, in one process, on n^3 cells of the trilinear box with a nodal field and a per-cell tensor set:

  - milliseconds of one call for each output alone, for all four together, of one cell_form call (no kappa,
    constrained: the same number as d_kappa) and of one pmg_laplacian_apply of the same operator; the ratio of all four
    to cell_form, and of d_field alone to d_kappa alone -- the price of the atomics;
  - the kernel's registers, spills and LDS at the degree, from the compiler's remarks (tools/kernel_resources.py);
  - with --write, the lines appended to profiles/form_gradients.md under a heading that names the run.

usage: python tools/form_gradients.py [--n 64] [--degree 4 | --degree 4,1,2] [--reps 20] [--rounds 5] [--write]
                                      [--resources-only | --no-resources]

Timing as tools/cell_form.py (measuring-on-mi355x): warm-up first; the calls alternate within every round, `reps`
back-to-back calls bracketed by HIP events per timing; the median over the rounds is reported with the smallest and
largest round.  No threshold: nobody has measured this kernel, or the atomic d_field sum on this access shape, before."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402
from cell_form import events, rotating_tensor, spread  # noqa: E402

NAMES = ("kappa", "field", "tensor", "sigma")


def resources(degrees):
    rows = kernel_resources.resource_rows("form_gradients.hip")
    lines = [kernel_resources.HEADER]
    for P in degrees:
        for name, r in rows.items():
            if re.search(rf"form_gradients_kernelILi{P + 1}E", name):
                lines.append(kernel_resources.table_row(f"form_gradients_kernel<{P + 1}> (degree {P})", r))
    return lines


def measure(a, P, lines):
    import torch

    import pmg_dolfinx_amd as pm

    part = pm.BoxPartition(a.n)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker, layout)
    gen = torch.Generator(device="cuda").manual_seed(0)
    n = layout.total
    kq = pm.Vector(layout)
    kq.data.copy_(1.0 + torch.rand(n, dtype=torch.float64, device="cuda", generator=gen))
    op.set_coefficient_field(kq)
    op.set_coefficient_tensor(rotating_tensor(part.xgeom[part.geom_dofmap].mean(axis=1)))
    x, v, y = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
    for t in (x, v):
        t.data.copy_(torch.randn(n, dtype=torch.float64, device="cuda", generator=gen))
    out = {"kappa": torch.empty(part.ncells, dtype=torch.float64, device="cuda"),
           "field": torch.empty(n, dtype=torch.float64, device="cuda"),
           "tensor": torch.empty((part.ncells, 6), dtype=torch.float64, device="cuda"),
           "sigma": torch.empty(part.ncells, dtype=torch.float64, device="cuda")}
    e = torch.empty(part.ncells, dtype=torch.float64, device="cuda")
    calls = {k: (lambda k=k: op.form_gradients(x, v, out={k: out[k]}, **{k: True})) for k in NAMES}
    calls["all four"] = lambda: op.form_gradients(x, v, out=out, kappa=True, field=True, tensor=True, sigma=True)
    calls["cell_form"] = lambda: op.cell_form(x, v, out=e, kappa=False, constrained=True)
    calls["apply"] = lambda: op(x, y)
    for _ in range(3):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t[k].append(events(torch, fn, a.reps))
    med = {k: statistics.median(val) for k, val in t.items()}
    # the Euler identity, as a check that the timed calls computed something: kq . d_field = kappa . d_kappa (kappa = 2)
    calls["all four"]()
    s_kappa, s_field = 2.0 * float(out["kappa"].sum()), float(kq.data @ out["field"])
    lines.append(f"degree {P}, {a.n}^3 cells ({n} dofs), nodal field and tensor set: "
                 + ", ".join(f"d_{k} alone {spread(t[k])}" for k in NAMES)
                 + f", all four {spread(t['all four'])}, cell_form {spread(t['cell_form'])}, apply {spread(t['apply'])}; "
                 f"all four / cell_form {med['all four'] / med['cell_form']:.3f}, "
                 f"d_field alone / d_kappa alone {med['field'] / med['kappa']:.3f}, "
                 f"all four / apply {med['all four'] / med['apply']:.3f}; sum_c kappa_c d_kappa = {s_kappa:.15e}, "
                 f"sum_n kq_n d_field = {s_field:.15e}, relative difference {abs(s_kappa - s_field) / abs(s_kappa):.2e}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--degree", default="4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/form_gradients.md")
    ap.add_argument("--resources-only", action="store_true", help="the compiler's table only (no GPU needed)")
    ap.add_argument("--no-resources", action="store_true", help="the times only (no compiler needed)")
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
    table = [] if a.no_resources else resources(degrees)
    print("\n".join(table))
    if a.write:
        path = os.path.join(ROOT, "profiles", "form_gradients.md")
        with open(path, "a") as f:
            f.write(f"\n## Run: `python tools/form_gradients.py {' '.join(sys.argv[1:])}`\n\n")
            f.write("".join(f"- {l}\n" for l in lines) + "\n" + "\n".join(table) + "\n")
        print("appended to", path)


if __name__ == "__main__":
    main()
