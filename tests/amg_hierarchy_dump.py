"""Child process of tests/test_gpu_amg_setup.py: build the AMG hierarchy of the twisted n^3 mesh in THIS process
(the library reads PMG_HOST_THREADS once per process) and write every exported array and every smoothing bound as
bytes.  Usage: python amg_hierarchy_dump.py N OUTPUT"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def hierarchy_bytes(amg):
    """rowptr, colidx, values of every A_l, then of every P_l, then the bounds."""
    L = amg.num_levels()
    mats = [amg.export(l, "A") for l in range(L)] + [amg.export(l, "P") for l in range(L - 1)]
    blob = b"".join(a.tobytes() for M in mats for a in (M.indptr, M.indices, M.data))
    return blob + np.array([amg.level_info(l)["lambda_max"] for l in range(L)]).tobytes()


def main(n, out):
    import torch

    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(1)
    layout = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    amg = pm.AmgSolver(op)
    with open(out, "wb") as f:
        f.write(hierarchy_bytes(amg))
    print("levels", [i["rows"] for i in amg.info()])


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
