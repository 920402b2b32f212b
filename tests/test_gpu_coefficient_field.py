"""Nodal diffusion coefficient (pmg_laplacian_set_coefficient_field): -div(kappa[cell] * kq(x) grad u).

The CPU truth is the oracle's operator with its stored tensor scaled point by point, ``A.G *= kq[A.dofmap][:, :, None]``
(pinned from first principles in tests/test_coefficient_field_abi.py); its Chebyshev, CG and multigrid classes then work
on it as they stand.  Tolerances are those of tests/test_gpu_parity.py on max|a-b| / max|b|: 1e-12 for an apply and
the diagonal, 1e-13 for the tensor, 1e-10 after a smoother or a V-cycle.

What is compared bit for bit is the stored tensor: it is written once per point, in a fixed order.  Two applications
of ONE operator on ONE tensor do not give the same bits -- the cell sums of a patch meet in LDS, and the patches of a
merged launch in memory, in whatever order the wavefronts arrive (measured on an MI355X on the unchanged kernels, no
field anywhere: P = 4 on (4, 4, 8) cells and P = 2 on (4, 4, 16), 200 of 200 repeated applies differ from the first in
some bit, merged and coloured launches alike; P = 2 on (3, 2, 4), 185 of 200).  Where "the apply is unchanged" is
checked next to equal tensor bits, the bound is therefore NOISE = 1e-14, the one tests/test_gpu_parity.py
(test_merged_and_coloured_launches_agree) uses for two runs of one operator.  The two tests that compare two applies
with ``torch.equal`` (test_clear_restores_the_apply_bit_for_bit, test_batched_apply_is_bit_identical_to_resident) use
a vector for which the order of the sums cannot matter, _order_free_vector."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def smooth_field(c):
    """1 + 0.5 sin(2 pi x) cos(2 pi y) + z at the dof coordinates: in [0.5, 2.5] on the unit cube."""
    return 1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1]) + c[:, 2]


def random_field(n, seed):
    """Seeded nodal values in [0.5, 2]: no symmetry for a wrong gather index to hide behind."""
    return np.random.default_rng(seed).uniform(0.5, 2.0, n)


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


NOISE = 1e-14  # two applications of one operator on the same tensor bits (see the module docstring)


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _scaled_oracle(P, kappa, dofmap, part, bc, kq):
    """The oracle's operator of -div(kappa kq grad u): its tensor scaled by the field at each point's dof."""
    from oracle import pmg_oracle as po

    A = po.Laplacian(P, kappa, dofmap, part.xgeom, part.geom_dofmap, bc)
    if kq is not None:
        A.G *= kq[A.dofmap][:, :, None]
        A._diag = None
    return A


def _level(pm, n, P, wf, kappa=2.0, coloured=False, **kw):
    part = pm.BoxPartition(n, warp=wf)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    try:
        if coloured:
            pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout, **kw)
    finally:
        if coloured:
            pm.set_merge_threshold(-1)
    return part, lv, layout, op


def _order_free_vector(P, lv, seed):
    """A vector whose apply has ONE bit pattern whatever order the cell sums arrive in.  It is non-zero only on
    cell-interior nodes (which belong to one cell) of a set of "active" cells chosen so that no mesh vertex -- hence
    no edge, face or dof -- touches more than two of them.  Every other cell contributes exact zeros, so each output
    entry is 0 + a + b with at most two non-zero terms: x + 0 is exact and a + b = b + a in IEEE arithmetic.  The
    active cells are about a quarter of the mesh; the tensor of every cell is compared bit for bit separately."""
    nd = P + 1
    dm = np.asarray(lv.dofmap).reshape(-1, nd**3)
    corners = [(a * nd + b) * nd + c for a in (0, P) for b in (0, P) for c in (0, P)]
    inner = [(a * nd + b) * nd + c for a in range(1, P) for b in range(1, P) for c in range(1, P)]
    touching = np.zeros(lv.ndofs, dtype=np.int64)
    rng = np.random.default_rng(seed)
    u = np.zeros(lv.ndofs)
    active = []
    for cell in range(dm.shape[0]):
        if np.all(touching[dm[cell, corners]] < 2):
            touching[dm[cell, corners]] += 1
            active.append(cell)
            u[dm[cell, inner]] = rng.standard_normal(len(inner))
    hits = np.bincount(dm[active].ravel(), minlength=lv.ndofs)
    assert hits.max() == 2 and len(active) >= dm.shape[0] // 8  # faces shared by two active cells are in
    return u


def _apply(pm, op, layout, u, fill=7.0):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(fill)
    op(x, y)
    return y


def _diag(pm, op, layout):
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    return d.data_copy()


# ---- 1. apply, tensor and diagonal, every degree ---------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_apply_tensor_diagonal_all_degrees(pm, P):
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=twist)
    kappa = np.random.default_rng(300 + P).uniform(1.0, 3.0, part.ncells)  # not constant: both factors are seen
    part, lv, layout, op = _level(pm, n, P, twist, kappa=kappa)
    kq = random_field(lv.ndofs, 200 + P)
    assert not op.has_coefficient_field()
    op.set_coefficient_field(_vec(pm, layout, kq))
    assert op.has_coefficient_field()
    A = _scaled_oracle(P, kappa, lv.dofmap, part, lv.bc_marker, kq)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    assert _relerr(_apply(pm, op, layout, u).data_copy(), A.apply(u)) < 1e-12
    assert _relerr(op.geometry().cpu().numpy(), A.G) < 1e-13
    op.compute_diag_inverse()
    assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    # the field is really in: the operator without it is another one
    A0 = _scaled_oracle(P, kappa, lv.dofmap, part, lv.bc_marker, None)
    assert _relerr(A0.apply(u), A.apply(u)) > 1e-2


# ---- 2. full patches, structured path ---------------------------------------------------------------------------


@pytest.mark.parametrize("P,n", [(1, (8, 8, 16)), (2, (4, 4, 16)), (3, (4, 4, 8)), (4, (4, 4, 8)), (5, (4, 4, 14)),
                                 (6, (2, 4, 8)), (7, (2, 2, 6)), (8, (2, 2, 6))])
def test_apply_full_patches(pm, P, n):
    part, lv, layout, op = _level(pm, n, P, None)
    kq = smooth_field(part.dof_coordinates(P))
    assert kq.min() >= 0.5 and kq.max() <= 2.5
    op.set_coefficient_field(_vec(pm, layout, kq))
    A = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq)
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(-3.0)
    op(x, y)
    assert _relerr(y.data_copy(), A.apply(u)) < 1e-12
    op(x, y)  # second application: no dependence on the previous content of y
    assert _relerr(y.data_copy(), A.apply(u)) < 1e-12


# ---- 3. set, change, clear --------------------------------------------------------------------------------------


def test_set_change_clear(pm):
    P, n = 4, (4, 4, 8)
    part, lv, layout, op = _level(pm, n, P, twist, coloured=True)
    u = np.random.default_rng(3).standard_normal(lv.ndofs)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    op(x, y)
    before = y.data.clone()
    g_before = op.geometry().clone()
    op.compute_diag_inverse()
    d_before = _diag(pm, op, layout)
    fields = (smooth_field(part.dof_coordinates(P)), random_field(lv.ndofs, 31))
    for kq in fields:
        op.set_coefficient_field(_vec(pm, layout, kq))
        A = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq)
        y.set(1.0)
        op(x, y)
        assert _relerr(y.data_copy(), A.apply(u)) < 1e-12
        # the inverse diagonal has followed, without another compute_diag_inverse
        assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    op.set_coefficient_field(None)
    assert not op.has_coefficient_field()
    A = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, None)
    y.set(1.0)
    op(x, y)
    assert _relerr(y.data_copy(), A.apply(u)) < 1e-12
    assert torch.equal(op.geometry(), g_before)  # today's tensor, bit for bit
    assert _relerr(y.data_copy(), before.cpu().numpy()) < NOISE
    assert _relerr(_diag(pm, op, layout), d_before) < 1e-14  # recomputed: its atomics arrive in any order
    op.set_coefficient_field(None)  # nothing to remove: no error
    # a diagonal installed by the caller is not overwritten
    mine = np.random.default_rng(5).uniform(0.1, 1.0, lv.ndofs)
    op.set_diag_inverse(_vec(pm, layout, mine))
    op.set_coefficient_field(_vec(pm, layout, fields[0]))
    assert np.array_equal(_diag(pm, op, layout), mine)
    op.set_coefficient_field(None)
    assert np.array_equal(_diag(pm, op, layout), mine)


def test_clear_restores_the_apply_bit_for_bit(pm):
    """After field A, field B and None, the apply equals, with ``torch.equal``, an apply made before any field was
    set.  The vector is one whose apply has a fixed bit pattern (_order_free_vector); a dense vector is compared at
    NOISE in test_set_change_clear."""
    P, n = 4, (4, 4, 8)
    part, lv, layout, op = _level(pm, n, P, twist, coloured=True)
    u = _order_free_vector(P, lv, 3)
    before = _apply(pm, op, layout, u).data.clone()
    assert torch.equal(_apply(pm, op, layout, u).data, before)  # the premise: this vector's apply is reproducible
    for kq in (smooth_field(part.dof_coordinates(P)), random_field(lv.ndofs, 31)):
        op.set_coefficient_field(_vec(pm, layout, kq))
        assert not torch.equal(_apply(pm, op, layout, u).data, before)  # ... and it sees the field
    op.set_coefficient_field(None)
    after = _apply(pm, op, layout, u).data
    print(f"apply after clearing the field vs before any field: {_relerr(after.cpu().numpy(), before.cpu().numpy()):.3e}")
    assert torch.equal(after, before)


# ---- 4. node order ----------------------------------------------------------------------------------------------


def test_basix_node_order(pm):
    P, n = 3, (3, 2, 4)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    perm = pm.basix_node_permutation(P)
    dm_basix = pm.dofmap_in_node_order(lv.dofmap, perm)
    op = pm.MatFreeLaplacian(P, 2.0, dm_basix, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout, node_order="basix")
    kq = random_field(lv.ndofs, 44)  # by dof number: no cell-local order involved
    op.set_coefficient_field(_vec(pm, layout, kq))
    A = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq)  # the oracle never sees the basix order
    u = np.random.default_rng(43).standard_normal(lv.ndofs)
    assert _relerr(_apply(pm, op, layout, u).data_copy(), A.apply(u)) < 1e-12
    p3 = pm.cell_permutation(perm)  # the tensor comes back indexed by the caller's point numbers
    assert _relerr(op.geometry().cpu().numpy(), A.G[:, p3, :]) < 1e-13
    op.compute_diag_inverse()
    assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12


# ---- 5. batched geometry ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("field_first", [True, False])
def test_batched_geometry(pm, field_first):
    from pmg_dolfinx_amd import _lib

    P, n = 2, (4, 4, 16)
    part, lv, layout, res = _level(pm, n, P, twist, coloured=True)
    _, _, _, bat = _level(pm, n, P, twist, coloured=True)
    kq = smooth_field(part.dof_coordinates(P))
    res.set_coefficient_field(_vec(pm, layout, kq))
    if field_first:
        bat.set_coefficient_field(_vec(pm, layout, kq))
    _lib.call("pmg_laplacian_set_geometry_batch", bat.handle, 8)  # the Python class refuses batching: the C entry point
    if not field_first:
        bat.set_coefficient_field(_vec(pm, layout, kq))
    A = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq)
    u = np.random.default_rng(8).standard_normal(lv.ndofs)
    yr, yb = _apply(pm, res, layout, u), _apply(pm, bat, layout, u)
    assert _relerr(yb.data_copy(), A.apply(u)) < 1e-12
    assert torch.equal(bat.geometry(), res.geometry())  # the recomputed batches hold the resident tensor's bits
    assert _relerr(yb.data_copy(), yr.data_copy()) < NOISE
    res.compute_diag_inverse()
    bat.compute_diag_inverse()
    assert _relerr(_diag(pm, bat, layout), A.diag_inverse()) < 1e-12
    assert _relerr(_diag(pm, bat, layout), _diag(pm, res, layout)) < 1e-14
    # back to the resident tensor: the field is still folded in
    _lib.call("pmg_laplacian_set_geometry_batch", bat.handle, 0)
    assert torch.equal(bat.geometry(), res.geometry())


def test_batched_apply_is_bit_identical_to_resident(pm):
    """The batched apply is bit-identical to the resident one with the same field, on a vector whose apply has a fixed
    bit pattern (_order_free_vector); a dense vector is compared at NOISE in test_batched_geometry."""
    from pmg_dolfinx_amd import _lib

    P, n = 2, (4, 4, 16)
    part, lv, layout, res = _level(pm, n, P, twist, coloured=True)
    _, _, _, bat = _level(pm, n, P, twist, coloured=True)
    kq = smooth_field(part.dof_coordinates(P))
    _lib.call("pmg_laplacian_set_geometry_batch", bat.handle, 8)
    u = _order_free_vector(P, lv, 8)
    plain = _apply(pm, res, layout, u).data.clone()
    for op in (res, bat):
        op.set_coefficient_field(_vec(pm, layout, kq))
    yr, yb = _apply(pm, res, layout, u), _apply(pm, bat, layout, u)
    print(f"batched vs resident apply with the field: {_relerr(yb.data_copy(), yr.data_copy()):.3e}")
    assert not torch.equal(yr.data, plain)  # the vector sees the field
    assert torch.equal(yb.data, yr.data)


# ---- 6. refusals ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_field", [False, True])
def test_invalid_entries_are_refused(pm, with_field):
    from pmg_dolfinx_amd import _lib

    P, n = 2, (3, 2, 4)
    part, lv, layout, op = _level(pm, n, P, twist, coloured=True)
    good = random_field(lv.ndofs, 61)
    if with_field:
        op.set_coefficient_field(_vec(pm, layout, good))
    op.compute_diag_inverse()
    u = np.random.default_rng(6).standard_normal(lv.ndofs)
    before = _apply(pm, op, layout, u).data.clone()
    g_before, d_before = op.geometry().clone(), _diag(pm, op, layout)
    for where, value in ((0, 0.0), (lv.ndofs // 2, -1.0), (lv.ndofs - 1, float("nan")), (7, float("inf"))):
        bad = good.copy()
        bad[where] = value
        with pytest.raises(_lib.PmgError, match="finite and greater than 0") as e:
            op.set_coefficient_field(_vec(pm, layout, bad))
        assert "(code -1)" in str(e.value)  # PMG_ERR_INVALID
        assert op.has_coefficient_field() == with_field
        assert torch.equal(op.geometry(), g_before)
        assert np.array_equal(_diag(pm, op, layout), d_before)
        assert _relerr(_apply(pm, op, layout, u).data_copy(), before.cpu().numpy()) < NOISE


def test_affine_mode_and_wrong_length_are_refused(pm):
    from pmg_dolfinx_amd import _lib

    P, n = 2, (3, 2, 4)
    part, lv, layout, op = _level(pm, n, P, None)
    assert op.is_affine()
    kq = _vec(pm, layout, smooth_field(part.dof_coordinates(P)))
    op.set_coefficient_field(kq)
    with pytest.raises(_lib.PmgError, match="pmg_laplacian_set_coefficient_field") as e:
        op.set_geometry_mode("affine")
    assert "(code -1)" in str(e.value)
    op.set_coefficient_field(None)
    op.set_geometry_mode("affine")
    with pytest.raises(_lib.PmgError, match="pmg_laplacian_set_geometry_mode") as e:
        op.set_coefficient_field(kq)
    assert "(code -1)" in str(e.value) and not op.has_coefficient_field()
    op.set_geometry_mode("stored")
    op.set_coefficient_field(kq)
    assert op.has_coefficient_field()
    # a Vector of another layout
    other = pm.Vector(pm.make_layout(part.level(1)))
    other.set(1.0)
    with pytest.raises(ValueError, match="entries"):
        op.set_coefficient_field(other)
    with pytest.raises(TypeError):
        op.set_coefficient_field(kq.data)


# ---- 7. FP32 ----------------------------------------------------------------------------------------------------


def _fp32_vs_fp64(pm, op, layout, u32):
    x = torch.from_numpy(u32).cuda()
    y = torch.full_like(x, 7.0)
    op.apply_fp32(x, y)
    torch.cuda.synchronize()
    ref = _apply(pm, op, layout, u32.astype(np.float64)).data_copy()
    return _relerr(y.cpu().numpy().astype(np.float64), ref), ref


@pytest.mark.parametrize("P", [4, 1])
def test_fp32_apply(pm, P):
    """apply_fp32 against the FP64 apply of the same operator.  The bound is the same error measured on the same mesh
    without a field, times 2: the field adds one rounding per point and has a 5:1 range."""
    n = (4, 4, 8)
    part, lv, layout, plain = _level(pm, n, P, twist)
    u32 = np.random.default_rng(70 + P).standard_normal(lv.ndofs).astype(np.float32)
    e0, y_plain = _fp32_vs_fp64(pm, plain, layout, u32)
    assert 0 < e0 < 1e-5
    kq = _vec(pm, layout, smooth_field(part.dof_coordinates(P)))
    # the field set before the first FP32 use ...
    _, _, _, early = _level(pm, n, P, twist)
    early.set_coefficient_field(kq)
    e1, y_field = _fp32_vs_fp64(pm, early, layout, u32)
    assert _relerr(y_field, y_plain) > 1e-2  # (the FP64 side has the field)
    assert e1 <= 2 * e0, f"fp32 vs fp64 with the field set first {e1:.3e}, without a field {e0:.3e}"
    # ... and on an operator that has already applied in FP32 (its float tensor exists)
    plain.set_coefficient_field(kq)
    e2, y_late = _fp32_vs_fp64(pm, plain, layout, u32)
    assert _relerr(y_late, y_field) < 1e-13
    assert e2 <= 2 * e0, f"fp32 vs fp64 with the field set after FP32 use {e2:.3e}, without a field {e0:.3e}"
    plain.set_coefficient_field(None)
    e3, y_again = _fp32_vs_fp64(pm, plain, layout, u32)
    assert _relerr(y_again, y_plain) < 1e-13 and e3 <= 2 * e0, (e3, e0)


# ---- 8. assembled operator --------------------------------------------------------------------------------------


def test_assembled_operator_follows_the_field(pm):
    P, n = 3, (3, 2, 2)
    part, lv, layout, op = _level(pm, n, P, twist)
    kq = smooth_field(part.dof_coordinates(P))
    op.set_coefficient_field(_vec(pm, layout, kq))
    M = pm.MatrixOperator(op)
    ref = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq).assemble_csr()
    assert abs(M.to_scipy() - ref).max() < 1e-12 * abs(ref).max()
    kq2 = random_field(lv.ndofs, 81)
    op.set_coefficient_field(_vec(pm, layout, kq2))
    assert abs(M.to_scipy() - ref).max() < 1e-12 * abs(ref).max()  # the matrix holds the values it was assembled with
    M.update_values()
    ref2 = _scaled_oracle(P, 2.0, lv.dofmap, part, lv.bc_marker, kq2).assemble_csr()
    assert abs(M.to_scipy() - ref2).max() < 1e-12 * abs(ref2).max()
    assert abs(ref2 - ref).max() > 1e-2 * abs(ref).max()
    u = np.random.default_rng(82).standard_normal(lv.ndofs)
    ym, yf = pm.Vector(layout), _apply(pm, op, layout, u)
    M(_vec(pm, layout, u), ym)
    assert _relerr(ym.data_copy(), yf.data_copy()) < 1e-12


# ---- 9. cycle and solve -----------------------------------------------------------------------------------------


def _oracle_hierarchy(n, orders, k, kappa, wf):
    """The oracle's V-cycle on field-scaled operators, with their own eigenvalue estimates."""
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh(n, warp=wf)
    ops, sm, eigs = [], [], []
    for P in orders:
        A = po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P))
        A.G *= smooth_field(mesh.dof_coordinates(P))[A.dofmap][:, :, None]
        A._diag = None
        ops.append(A)
        rng, _ = po.estimate_eig_range(A, A.ndofs)
        eigs.append(rng)
        sm.append(po.Chebyshev(rng, k))
    it = [po.Interpolator(orders[i], orders[i + 1], ops[i].dofmap, ops[i + 1].dofmap, ops[i].ndofs, ops[i + 1].ndofs)
          for i in range(len(orders) - 1)]
    return mesh, ops, po.MultigridPreconditioner(ops, sm, it, mesh.boundary_marker(orders[0])), eigs


def test_vcycle_and_pcg(pm):
    from oracle import pmg_oracle as po

    n, orders, k = 4, (1, 2, 4), 3
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=k, warp=warp, kappa_field=smooth_field)
    assert all(op.has_coefficient_field() for op in h.operators)
    mesh, ops, mg, eigs = _oracle_hierarchy(n, orders, k, 2.0, warp)
    for got, ref in zip(h.eig_ranges, eigs):
        assert abs(got[1] - ref[1]) < 1e-8 * ref[1]
    b = h.rhs[-1].data_copy()  # the load keeps the per-cell kappa only
    assert _relerr(b, ops[-1].rhs_manufactured(mesh.dof_coordinates(orders[-1]))) < 1e-12
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)
    ref = mg.apply(b, np.zeros_like(b))
    err = _relerr(x.data_copy(), ref)
    print(f"V-cycle with a coefficient field vs oracle: {err:.3e}")
    assert err < 1e-10
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(50)
    cg.set_tolerance(1e-8)
    xs = h.new_vector()
    xs.set(0.0)
    its = cg.solve(h.operators[-1], xs, h.rhs[-1], preconditioner=h.mg)
    ocg = po.CGSolver()
    ocg.set_max_iterations(50)
    ocg.set_tolerance(1e-8)
    xo = np.zeros_like(b)
    oits = ocg.solve(ops[-1], xo, b, precond=lambda r: mg.apply(r, np.zeros_like(r)))
    print(f"PCG iterations with a coefficient field: {its}, oracle {oits}")
    assert abs(its - oits) <= 1 and oits < 50
    r = pm.Vector(h.layouts[-1])
    h.operators[-1](xs, r)
    pm.axpy(r, -1.0, r, h.rhs[-1])
    assert pm.norm(r) < 1e-6 * pm.norm(h.rhs[-1])  # it solves the system with the field


# ---- 10. AMG coarse level ---------------------------------------------------------------------------------------


def test_amg_coarse_level_reads_the_field(pm):
    n, orders = 6, (1, 2)
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=2, warp=warp, kappa_field=smooth_field)
    amg = pm.AmgSolver(h.operators[0], cycles=1)
    h.mg.set_coarse_solver(amg)
    x = h.new_vector()
    x.set(0.0)
    r0 = pm.norm(h.rhs[-1])
    r1 = h.mg.apply(h.rhs[-1], x, verbose=True)
    r2 = h.mg.apply(h.rhs[-1], x, verbose=True)
    assert r2 < r1 < r0, (r0, r1, r2)
    h.mg.set_coarse_solver(None)
    mesh, ops, mg, eigs = _oracle_hierarchy(n, orders, 2, 2.0, warp)
    ref = ops[0].assemble_csr()
    free = ~mesh.boundary_marker(1).astype(bool)
    A0 = amg.export(0, "A")
    assert abs(A0[free] - ref[free]).max() < 1e-12 * abs(ref).max()


# ---- 11. two ranks on one GPU -----------------------------------------------------------------------------------


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, args, timeout=120):
    """tests/test_gpu_distributed.py's launcher: `world` spawned processes report (rank, result) or (rank, traceback);
    on the first failure, a dead rank or the time limit every process is terminated and joined -- nothing further is
    started on the GPU."""
    import queue as _queue

    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        while len(res) < world:
            try:
                rank, out = q.get(timeout=5)
            except _queue.Empty:
                timeout -= 5
                dead = [i for i, p in enumerate(procs) if p.exitcode not in (None, 0) and i not in res]
                if dead:
                    raise AssertionError(f"rank(s) {dead} died without reporting (exit codes "
                                         f"{[procs[i].exitcode for i in dead]})")
                if timeout <= 0:
                    raise AssertionError("timed out waiting for the ranks")
                continue
            if isinstance(out, str):
                raise AssertionError(f"rank {rank} failed:\n{out}")
            res[rank] = out
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [res[r] for r in range(world)]


def _rank_body(rank, world, port, n, dims, P):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm
        from oracle import pmg_oracle as po

        torch.cuda.set_device(0)
        H = pm.PoissonHierarchy(n, (P,), kappa=2.0, proc_dims=dims, rank=rank, size=world, warp=warp)
        lv, layout, op = H.levels[0], H.layouts[0], H.operators[0]
        gm = po.BoxMesh(n, warp=warp)
        A = po.Laplacian(P, 2.0, gm.dofmap(P), gm.xgeom, gm.geom_dofmap, gm.boundary_marker(P))
        kq = random_field(A.ndofs, 111)  # global, by global dof number
        A.G *= kq[A.dofmap][:, :, None]
        A._diag = None
        own = lv.local_to_global[: lv.size_local]
        mine = np.full(lv.ndofs, np.nan)  # entries beyond size_local are not the caller's to fill
        mine[: lv.size_local] = kq[own]
        v = pm.Vector(layout)
        v.data.copy_(torch.from_numpy(mine))
        op.set_coefficient_field(v)  # the hierarchy computed the diagonal: it follows
        del v
        ug = np.random.default_rng(11).standard_normal(A.ndofs)
        xl = np.zeros(lv.ndofs)
        xl[: lv.size_local] = ug[own]
        x, y, d = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
        x.data.copy_(torch.from_numpy(xl))
        op(x, y)
        op.get_diag_inverse(d)
        ref, dref = A.apply(ug)[own], A.diag_inverse()[own]
        dist.barrier()
        return {"ghosts": int(lv.num_ghosts),
                "apply": float(np.abs(y.data_copy()[: lv.size_local] - ref).max() / np.abs(ref).max()),
                "diag": float(np.abs(d.data_copy()[: lv.size_local] - dref).max() / np.abs(dref).max())}
    finally:
        dist.destroy_process_group()


def _rank_worker(rank, world, port, *args):
    q = args[-1]
    try:
        q.put((rank, _rank_body(rank, world, port, *args[:-1])))
    except BaseException:  # noqa: BLE001 -- reported to the parent, which fails the test
        import traceback

        q.put((rank, traceback.format_exc()))
        raise


def test_two_ranks_scatter_the_field_themselves(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks(_rank_worker, 2, ((3, 4, 8), (1, 1, 2), 2))
    for out in res:
        assert out["ghosts"] > 0
        assert out["apply"] < 1e-12 and out["diag"] < 1e-12, out
