"""What the distributed assembled operator costs, on one GPU: one rank of a 1x1x2 split (n^3 owned cells + the ghost
layer) with the rank as its own halo partner through halo windows (tools/self_partner_cycle.py,
tools/time_exchange_overhead.py: the rehearsal of the multi-rank code path profiles/exchange_overhead_r04.txt used).

  1. per level: the split product (put / owned columns of all rows / get / ghost columns of the boundary rows) against
     the one-launch product over whole rows on the same matrix, and the matrix-free application;
  2. the 4 -> 2 -> 1 V-cycle with level 0 assembled against the same cycle matrix-free, eager and as a hipGraph.

On a commit without pmg_matrix_create_distributed only the matrix-free numbers are printed.
usage: python tools/matrix_distributed.py [n] [reps] [cycles]     (defaults 32, 200, 50)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pmg_dolfinx_amd as pm
from pmg_dolfinx_amd import problem

NC = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
CYCLES = int(sys.argv[3]) if len(sys.argv) > 3 else 50
ORDERS = (1, 2, 4)
torch.cuda.set_device(0)
native = pm.RcclComm(0, 1, pm.RcclComm.unique_id(), halo="windows")


def make(lv, group=None, device="cuda", comm=None):
    m = min(sum(lv.send_counts), sum(lv.recv_counts))
    return pm.Layout(lv.size_local, lv.num_ghosts, [0] if m else [], [m] if m else [], [m] if m else [],
                     lv.send_indices[:m], lv.recv_indices[:m], device=device, comm=native)


problem.make_layout = make


def timed(fn, reps):
    """microseconds per call: warm-up, then `reps` calls between two events"""
    for _ in range(max(3, reps // 10)):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


H = pm.PoissonHierarchy((NC, NC, 2 * NC), ORDERS, cheb_its=3, proc_dims=(1, 1, 2), rank=0, size=2)
print(f"one rank of 1x1x2, {NC}^3 owned cells, degrees {ORDERS}, self partner over halo windows; "
      f"owned dofs {[lv.size_local for lv in H.levels]}, ghosts {[lv.num_ghosts for lv in H.levels]}")
try:
    mats = [pm.MatrixOperator(op, distributed=True) for op in H.operators[:2]]
except TypeError:
    mats = []
    print("this commit has no distributed assembled operator: matrix-free numbers only")

for i, M in enumerate(mats):
    layout, op = H.layouts[i], H.operators[i]
    x, y = pm.Vector(layout), pm.Vector(layout)
    x.set(1.0)
    od, brows = M.export_split()
    rp = M.export()[0]
    free = timed(lambda: op(x, y), REPS)
    as_routed = timed(lambda: M(x, y), REPS)
    os.environ["PMG_FUSED_EXCHANGE"] = "0"  # no level takes its exchange whole: the split form
    split = timed(lambda: M(x, y), REPS)
    free_split = timed(lambda: op(x, y), REPS)
    del os.environ["PMG_FUSED_EXCHANGE"]
    one = timed(lambda: M.apply_ghosts_current(x, y), REPS)
    scatter = timed(lambda: x.scatter_fwd(), REPS)
    print(f"level {i} (degree {ORDERS[i]}): rows {M.rows}, nnz {M.nnz}, boundary rows {brows.size}, off-diag entries "
          f"{int((rp[1:] - od).sum())}")
    print(f"  product, split (put / diag / get / off-diag): {split:8.2f} us")
    print(f"  product, as routed (whole exchange + one launch where the level is merged): {as_routed:8.2f} us")
    print(f"  product, one launch, no exchange:             {one:8.2f} us")
    print(f"  forward scatter alone:                        {scatter:8.2f} us")
    print(f"  matrix-free application, as routed / split:   {free:8.2f} / {free_split:.2f} us")


def cycle(graph):
    H.mg.set_graph(graph)
    x = H.new_vector()
    x.set(0.0)
    t = timed(lambda: H.mg.apply(H.rhs[-1], x), CYCLES)
    return t * 1e-3


for name, levels in (("matrix-free", ()), ("level 0 assembled", (0,)), ("levels 0, 1 assembled", (0, 1))):
    if levels and not mats:
        continue
    for i in range(len(mats)):
        H.mg.set_level_matrix(i, mats[i] if i in levels else None)
    print(f"cycle, {name}: eager {cycle(False):.3f} ms, hipGraph {cycle(True):.3f} ms per cycle; "
          f"applications per cycle {H.mg.apply_counts()}")
