"""Record, bit for bit, what the geometry code of a build computes, and compare two such records.

  python tools/operator_data_bits.py --out DIR     one DIR/<mesh>.npz per mesh case, with the library PMG_AMD_LIB names
                                                   (default: the tree's own)
  python tools/operator_data_bits.py --compare DIR_A DIR_B
                                                   every array of every file: identical, or the number of entries that
                                                   differ and the largest difference in ulps of the entry

Mesh cases: a box, a skewed (sheared, still affine) box, the box with every cell in a frame drawn from all 48
(left-handed cells included), and a mesh with a coordinate element of degree 2 on the quarter annulus.  Degrees P = 2, 4,
5, with a nodal field and a per-cell tensor set.  Per mesh and degree:

  G, G_batched   the exported tensor (pmg_laplacian_get_geometry), resident and in batched-geometry mode, on 3 x 2 x 5
                 cells: each point is written by one thread
  on a column of 1 x 1 x 6 cells, where a dof belongs to at most two cells and two patches, so every atomic sum has two
  terms and does not depend on their order:
  affine         an apply in affine mode (Gaff; tensor set, no field; where the cells are affine)
  fp32           an FP32 apply (the float tensor)
  rhs, lifting   the load vector and the Dirichlet lifting of b = 0
  reaction       the reaction vector, read through y = A 1 + d .* 1 of an operator with kappa = 1e-30

The arrays are compared by value bits, not the files byte by byte: an .npz carries the time it was written."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

DEGREES = (2, 4, 5)
MESHES = ("box", "skewed", "left_handed", "g2")


def skew(x):
    return np.stack([x[:, 0] + 0.3 * x[:, 1] + 0.1 * x[:, 2], x[:, 1] + 0.2 * x[:, 2], x[:, 2]], axis=1)


def quarter_annulus(x):
    r, t = 1.0 + x[:, 0], 0.5 * np.pi * x[:, 1]
    return np.stack([r * np.cos(t), r * np.sin(t), x[:, 2]], axis=1)


def partition(pm, mesh, n):
    if mesh == "left_handed":
        frames = np.random.default_rng(int(np.prod(n))).integers(0, 48, n)
        assert {pm.cell_symmetries()[f][2] for f in frames.ravel()} == {-1, 1}
        return pm.BoxPartition(n, cell_frames=frames)
    if mesh == "g2":
        return pm.BoxPartition(n, warp=quarter_annulus, geom_degree=2)
    return pm.BoxPartition(n, warp=skew if mesh == "skewed" else None)


def spd(ncells, rng):
    out = np.empty((ncells, 6))
    for c in range(ncells):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        M = (Q * rng.uniform(0.5, 2.0, 3)) @ Q.T
        out[c] = [M[0, 0], 0.5 * (M[0, 1] + M[1, 0]), 0.5 * (M[0, 2] + M[2, 0]), M[1, 1], 0.5 * (M[1, 2] + M[2, 1]),
                  M[2, 2]]
    return out


def record(pm, mesh, P):
    import torch

    from pmg_dolfinx_amd import _lib

    out = {}

    def operator(n, marker=None, kappa=None):
        part = partition(pm, mesh, n)
        lv = part.level(P)
        layout = pm.make_layout(lv)
        rng = np.random.default_rng(1000 * P + part.ncells)
        bc = lv.bc_marker if marker is None else marker(part, lv)
        kappa = rng.uniform(0.5, 1.5, part.ncells) if kappa is None else np.full(part.ncells, kappa)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bc, layout,
                                 geometry_degree=part.geom_degree)
        return part, lv, layout, bc, op, rng

    def vec(layout, a):
        v = pm.Vector(layout)
        v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
        return v

    def apply(op, layout, u):
        y = pm.Vector(layout)
        y.set(7.0)
        op(vec(layout, u), y)
        return y.data_copy()

    # the exported tensor
    part, lv, layout, _, op, rng = operator((3, 2, 5))
    op.set_coefficient_field(vec(layout, rng.uniform(0.5, 2.0, lv.ndofs)))
    op.set_coefficient_tensor(spd(part.ncells, rng))
    out["G"] = op.geometry().cpu().numpy()
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 7)
    out["G_batched"] = op.geometry().cpu().numpy()

    # the column
    def z0(part, lv):
        straight = pm.BoxPartition(part.n, geom_degree=part.geom_degree).dof_coordinates(P)
        return (lv.bc_marker.astype(bool) & (np.abs(straight[:, 2]) < 1e-12)).astype(np.int8)

    part, lv, layout, bc, op, rng = operator((1, 1, 6), marker=z0)
    u = rng.standard_normal(lv.ndofs)
    op.set_coefficient_tensor(spd(part.ncells, rng))
    if op.is_affine():
        op.set_geometry_mode("affine")
        out["affine"] = apply(op, layout, u)
        op.set_geometry_mode("stored")
    op.set_coefficient_field(vec(layout, rng.uniform(0.5, 2.0, lv.ndofs)))
    x32 = torch.from_numpy(u.astype(np.float32)).cuda()
    y32 = torch.full_like(x32, 7.0)
    op.apply_fp32(x32, y32)
    torch.cuda.synchronize()
    out["fp32"] = y32.cpu().numpy()
    b = pm.Vector(layout)
    op.assemble_rhs(vec(layout, rng.standard_normal(lv.ndofs)), b)
    out["rhs"] = b.data_copy()
    b = vec(layout, np.zeros(lv.ndofs))  # (from zero: two terms per entry)
    op.apply_lifting(vec(layout, np.where(bc.astype(bool), rng.standard_normal(lv.ndofs), np.nan)), b)
    out["lifting"] = b.data_copy()
    # the reaction vector itself: with kappa = 1e-30 the stiffness part of y = A 1 + d .* 1 is absorbed by d, whose
    # entries come back bit for bit (an apply with kappa of order one would sum three terms per entry, in any order)
    part, lv, layout, bc, op, rng = operator((1, 1, 6), marker=z0, kappa=1e-30)
    op.set_reaction(rng.uniform(0.5, 4.0, part.ncells))
    out["reaction"] = apply(op, layout, np.ones(lv.ndofs))
    return out


def ulps(a, b):
    """Largest difference of two arrays of one float type in units in the last place of the entry; entries that differ."""
    bits = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    differ = a.view(bits) != b.view(bits)
    if not differ.any():
        return 0.0, 0
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(a))
    return float(np.nanmax(np.where(differ, d, 0.0))), int(differ.sum())


def compare(dir_a, dir_b):
    worst = 0.0
    for mesh in MESHES:
        fa, fb = (np.load(os.path.join(d, mesh + ".npz")) for d in (dir_a, dir_b))
        assert sorted(fa.files) == sorted(fb.files), (mesh, fa.files, fb.files)
        for name in sorted(fa.files):
            a, b = fa[name], fb[name]
            assert a.shape == b.shape and a.dtype == b.dtype, (mesh, name)
            if a.tobytes() == b.tobytes():
                print(f"{mesh}: {name} {a.shape} identical")
                continue
            u, n = ulps(a, b)
            worst = max(worst, u)
            print(f"{mesh}: {name} {a.shape} DIFFERS in {n} of {a.size} entries, by at most {u:.2f} ulp")
    print("all arrays identical" if worst == 0.0 else f"largest difference {worst:.2f} ulp")
    return 0 if worst == 0.0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    import torch

    import pmg_dolfinx_amd as pm
    from pmg_dolfinx_amd import _lib

    torch.cuda.set_device(0)
    os.makedirs(a.out, exist_ok=True)
    print(f"operator_data_bits: {torch.cuda.get_device_name(0)}, library {_lib.LIB_PATH}")
    for mesh in MESHES:
        arrays = {}
        for P in DEGREES:
            for name, v in record(pm, mesh, P).items():
                arrays[f"P{P}_{name}"] = v
        np.savez(os.path.join(a.out, mesh + ".npz"), **arrays)
        print(f"{mesh}: {len(arrays)} arrays")


if __name__ == "__main__":
    main()
