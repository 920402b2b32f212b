"""Per-cycle kernel times of the flagship V-cycle (64^3 cells, p = 4 -> 2 -> 1, Chebyshev(3)) from a rocprofv3 kernel
trace, with the fused restriction on or off: time and launches per cycle of every kernel family, and the idle time
between kernels.
usage (GPU box):  cd /tmp && rocprofv3 --kernel-trace --output-format csv -d OUT -- \\
                      python <repo>/tools/cycle_profile.py run [--fused -1|0] [--cycles 10] [--n 64]
                  python <repo>/tools/cycle_profile.py summarize OUT [cycles]
`run` ends with the timed cycles, so the trace ends with `cycles` repetitions of one launch sequence; `summarize` finds
that period and reduces those cycles only (set-up and warm-up kernels are left out)."""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(argv):
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", type=int, default=-1)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--n", type=int, default=64)
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import torch

    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    h = pm.PoissonHierarchy(a.n, (1, 2, 4), kappa=2.0, cheb_its=3)
    try:
        h.mg.set_fused_restriction(a.fused)
    except AttributeError:  # a library from before the switch (A/B runs through PMG_AMD_LIB)
        pass
    x = h.new_vector()
    x.set(0.0)
    for _ in range(3 + a.cycles):
        h.mg.apply(h.rhs[-1], x)
    torch.cuda.synchronize()
    try:
        fused = h.mg.fused_restrictions()
    except AttributeError:
        fused = 0
    print(f"cycles {a.cycles}, fused restrictions per cycle {fused}, apply counts {h.mg.apply_counts()}, "
          f"launches per apply {[op.launches_per_apply() for op in h.operators]}")


def family(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"(stiffness_restrict_kernel<\d, \d)|(stiffness_column_kernel<\d)|(restrict_patch_kernel<\d, \d)|"
                 r"(prolong_patch_kernel<\d, \d)|ew_kernel2<(Cheb\w+<[\w, ]+)|ew_kernel2<(\w+)|(\w+)", n)
    return next(g for g in m.groups() if g) if m else n[:40]


def summarize(argv):
    (path,) = glob.glob(os.path.join(argv[0], "**", "*kernel_trace.csv"), recursive=True)[:1]
    ncyc = int(argv[1]) if len(argv) > 1 else 10
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path)))
    names = [n for _, _, n in rows]
    period = next(p for p in range(8, len(names) // ncyc + 1)
                  if all(names[-ncyc * p + i] == names[-ncyc * p + i + p] for i in range((ncyc - 1) * p)))
    sel = rows[-ncyc * period:]
    span = sel[-1][1] - sel[0][0]
    busy, count = defaultdict(int), defaultdict(int)
    idle, last_end = 0, sel[0][0]
    for s, e, n in sel:
        f = family(n)
        busy[f] += e - s
        count[f] += 1
        idle += max(0, s - last_end)
        last_end = max(last_end, e)
    tot = sum(busy.values())
    print(f"{period} launches per cycle over {ncyc} cycles: span {span / ncyc * 1e-6:.3f} ms per cycle, kernel time "
          f"{tot / ncyc * 1e-6:.3f} ms, idle between kernels {idle / ncyc * 1e-3:.1f} us ({100 * idle / span:.1f} %)")
    for f, t in sorted(busy.items(), key=lambda kv: -kv[1]):
        print(f"  {f:34s} {count[f] / ncyc:6.1f} launches/cycle {t / ncyc * 1e-3:9.1f} us/cycle "
              f"{t / count[f] * 1e-3:8.1f} us/launch {100 * t / span:5.1f} %")


if __name__ == "__main__":
    {"run": run, "summarize": summarize}[sys.argv[1]](sys.argv[2:])
