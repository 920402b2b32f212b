"""Full-tensor diffusion (pmg_laplacian_set_coefficient_tensor): -div(kappa[cell] * kq(x) * K[cell] grad u) with K
symmetric positive definite per cell.

The CPU truth is the oracle's operator with its stored tensor replaced by adj(J) K adj(J)^T w / det J
(tests/tensor_coefficient_reference.py, pinned from first principles in tests/test_coefficient_tensor_abi.py); the
oracle's Chebyshev, CG and multigrid classes then work on it as they stand.  Tolerances are those of
tests/test_gpu_parity.py and tests/test_gpu_coefficient_field.py on max|a-b| / max|b|: 1e-12 for an apply, the diagonal
and CSR values, 1e-13 for the tensor, 1e-10 after a smoother or a V-cycle, NOISE = 1e-14 for two applications of one
operator on the same tensor bits (their sums arrive in any order, see the field's test file).  ``torch.equal`` is used
only on the stored tensor, which is written once per point in a fixed order, and on applies of that file's
``_order_free_vector``."""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tensor_coefficient_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NOISE = 1e-14
SHEAR = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def shear(x):
    return x @ SHEAR.T


def random_field(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, n)


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _level(pm, n, P, wf, kappa=2.0, coloured=False, bc=None):
    part = pm.BoxPartition(n, warp=wf)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    try:
        if coloured:
            pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                 lv.bc_marker if bc is None else bc, layout)
    finally:
        if coloured:
            pm.set_merge_threshold(-1)
    return part, lv, layout, op


def _oracle(P, kappa, part, lv, T=None, kq=None, bc=None):
    A = tr.laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker if bc is None else bc)
    if T is not None:
        tr.with_tensor(A, T, kq)
    return A


def _centres(part):
    return tr.cell_centres(part.xgeom, part.geom_dofmap)


def _apply(pm, op, layout, u, fill=7.0):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(fill)
    op(x, y)
    return y


def _diag(pm, op, layout):
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    return d.data_copy()


def _order_free_vector(P, lv, seed):
    """tests/test_gpu_coefficient_field.py's vector whose apply has ONE bit pattern whatever order the cell sums arrive
    in: non-zero only on cell-interior nodes of "active" cells of which no mesh vertex touches more than two, so each
    output entry is 0 + a + b with at most two non-zero terms."""
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
    assert hits.max() == 2 and len(active) >= dm.shape[0] // 8
    return u


# ---- 1. apply, tensor and diagonal, every degree ---------------------------------------------------------------


@pytest.mark.parametrize("P,with_field", [(P, False) for P in range(1, 9)] + [(2, True), (4, True)])
def test_apply_tensor_diagonal_all_degrees(pm, P, with_field):
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=twist)
    kappa = np.random.default_rng(300 + P).uniform(1.0, 3.0, part.ncells)
    part, lv, layout, op = _level(pm, n, P, twist, kappa=kappa)
    T = tr.random_spd(part.ncells, 400 + P)
    kq = random_field(lv.ndofs, 200 + P) if with_field else None
    assert not op.has_coefficient_tensor()
    if with_field:
        op.set_coefficient_field(_vec(pm, layout, kq))
    op.set_coefficient_tensor(T)
    assert op.has_coefficient_tensor() and op.has_coefficient_field() == with_field
    A = _oracle(P, kappa, part, lv, T, kq)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    assert _relerr(_apply(pm, op, layout, u).data_copy(), A.apply(u)) < 1e-12
    assert _relerr(op.geometry().cpu().numpy(), A.G) < 1e-13
    op.compute_diag_inverse()
    assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    # the tensor is really in: the scalar operator is another one
    A0 = _oracle(P, kappa, part, lv)
    assert _relerr(A0.apply(u), A.apply(u)) > 1e-2
    # a device tensor is taken as it is
    op.set_coefficient_tensor(torch.from_numpy(T).cuda())
    assert _relerr(op.geometry().cpu().numpy(), A.G) < 1e-13


# ---- 2. full patches, structured path ---------------------------------------------------------------------------


@pytest.mark.parametrize("P,n", [(1, (8, 8, 16)), (2, (4, 4, 16)), (3, (4, 4, 8)), (4, (4, 4, 8)), (5, (4, 4, 14)),
                                 (6, (2, 4, 8)), (7, (2, 2, 6)), (8, (2, 2, 6))])
def test_apply_full_patches(pm, P, n):
    part, lv, layout, op = _level(pm, n, P, None)
    T = tr.rotating_tensor(_centres(part))
    op.set_coefficient_tensor(T)
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    ref = _oracle(P, 2.0, part, lv, T).apply(u)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(-3.0)
    op(x, y)
    assert _relerr(y.data_copy(), ref) < 1e-12
    op(x, y)  # second application: no dependence on the previous content of y
    assert _relerr(y.data_copy(), ref) < 1e-12


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
    tensors = (tr.rotating_tensor(_centres(part)), tr.random_spd(part.ncells, 31))
    for T in tensors:
        op.set_coefficient_tensor(T)
        A = _oracle(P, 2.0, part, lv, T)
        y.set(1.0)
        op(x, y)
        assert _relerr(y.data_copy(), A.apply(u)) < 1e-12
        # the inverse diagonal has followed, without another compute_diag_inverse
        assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    op.set_coefficient_tensor(None)
    assert not op.has_coefficient_tensor()
    y.set(1.0)
    op(x, y)
    assert _relerr(y.data_copy(), _oracle(P, 2.0, part, lv).apply(u)) < 1e-12
    assert torch.equal(op.geometry(), g_before)  # today's tensor, bit for bit
    assert _relerr(y.data_copy(), before.cpu().numpy()) < NOISE
    assert _relerr(_diag(pm, op, layout), d_before) < 1e-14  # recomputed: its atomics arrive in any order
    op.set_coefficient_tensor(None)  # nothing to remove: no error
    assert torch.equal(op.geometry(), g_before)
    # a diagonal installed by the caller is not overwritten
    mine = np.random.default_rng(5).uniform(0.1, 1.0, lv.ndofs)
    op.set_diag_inverse(_vec(pm, layout, mine))
    op.set_coefficient_tensor(tensors[0])
    assert np.array_equal(_diag(pm, op, layout), mine)
    op.set_coefficient_tensor(None)
    assert np.array_equal(_diag(pm, op, layout), mine)


def test_clear_restores_the_apply_bit_for_bit(pm):
    P, n = 4, (4, 4, 8)
    part, lv, layout, op = _level(pm, n, P, twist, coloured=True)
    u = _order_free_vector(P, lv, 3)
    before = _apply(pm, op, layout, u).data.clone()
    assert torch.equal(_apply(pm, op, layout, u).data, before)  # the premise: this vector's apply is reproducible
    for T in (tr.rotating_tensor(_centres(part)), tr.random_spd(part.ncells, 31)):
        op.set_coefficient_tensor(T)
        assert not torch.equal(_apply(pm, op, layout, u).data, before)  # ... and it sees the tensor
    op.set_coefficient_tensor(None)
    assert torch.equal(_apply(pm, op, layout, u).data, before)


# ---- 4. affine mode ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 4, 6])
def test_affine_mode_carries_the_tensor(pm, P):
    n = (4, 4, 8) if P <= 4 else (2, 2, 4)
    part, lv, layout, op = _level(pm, n, P, shear)
    assert op.is_affine()
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    T = tr.random_spd(part.ncells, 50 + P)
    ref = _oracle(P, 2.0, part, lv, T).apply(u)
    # set in stored mode, then switched
    op.set_coefficient_tensor(T)
    stored = _apply(pm, op, layout, u).data_copy()
    assert _relerr(stored, ref) < 1e-12
    op.set_geometry_mode("affine")
    got = _apply(pm, op, layout, u).data_copy()
    assert _relerr(got, ref) < 1e-12 and _relerr(got, stored) < 1e-12
    # cleared in affine mode: the plain affine apply
    op.set_coefficient_tensor(None)
    _, _, _, op0 = _level(pm, n, P, shear)
    op0.set_geometry_mode("affine")
    plain_affine = _apply(pm, op0, layout, u).data_copy()
    assert _relerr(_apply(pm, op, layout, u).data_copy(), plain_affine) < NOISE
    assert _relerr(plain_affine, ref) > 1e-2
    # set while in affine mode, with other values
    T2 = tr.rotating_tensor(_centres(part))
    ref2 = _oracle(P, 2.0, part, lv, T2).apply(u)
    op.set_coefficient_tensor(T2)
    got2 = _apply(pm, op, layout, u).data_copy()
    assert _relerr(got2, ref2) < 1e-12
    op.set_geometry_mode("stored")
    assert _relerr(got2, _apply(pm, op, layout, u).data_copy()) < 1e-12
    # the refusal that remains is the nodal field's
    op.set_geometry_mode("affine")
    with pytest.raises(pm._lib.PmgError, match="pmg_laplacian_set_coefficient_field"):
        op.set_coefficient_field(_vec(pm, layout, random_field(lv.ndofs, 1)))


# ---- 5. batched geometry ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("tensor_first", [True, False])
def test_batched_geometry(pm, tensor_first):
    from pmg_dolfinx_amd import _lib

    P, n = 2, (4, 4, 16)
    part, lv, layout, res = _level(pm, n, P, twist, coloured=True)
    _, _, _, bat = _level(pm, n, P, twist, coloured=True)
    T = tr.rotating_tensor(_centres(part))
    res.set_coefficient_tensor(T)
    if tensor_first:
        bat.set_coefficient_tensor(T)
    _lib.call("pmg_laplacian_set_geometry_batch", bat.handle, 8)  # the Python class refuses batching: the C entry point
    if not tensor_first:
        bat.set_coefficient_tensor(T)
    A = _oracle(P, 2.0, part, lv, T)
    u = np.random.default_rng(8).standard_normal(lv.ndofs)
    yr, yb = _apply(pm, res, layout, u), _apply(pm, bat, layout, u)
    assert _relerr(yb.data_copy(), A.apply(u)) < 1e-12
    assert torch.equal(bat.geometry(), res.geometry())  # the recomputed batches hold the resident tensor's bits
    assert _relerr(yb.data_copy(), yr.data_copy()) < NOISE
    uo = _order_free_vector(P, lv, 8)
    assert torch.equal(_apply(pm, bat, layout, uo).data, _apply(pm, res, layout, uo).data)
    res.compute_diag_inverse()
    bat.compute_diag_inverse()
    assert _relerr(_diag(pm, bat, layout), A.diag_inverse()) < 1e-12
    # back to the resident tensor: the coefficient is still folded in
    _lib.call("pmg_laplacian_set_geometry_batch", bat.handle, 0)
    assert torch.equal(bat.geometry(), res.geometry())
    assert _relerr(_apply(pm, bat, layout, u).data_copy(), yr.data_copy()) < NOISE
    assert torch.equal(_apply(pm, bat, layout, uo).data, _apply(pm, res, layout, uo).data)


# ---- 6. chain form ----------------------------------------------------------------------------------------------


def test_chain_form(pm, monkeypatch):
    P, n = 4, (4, 4, 64)
    monkeypatch.setenv("PMG_CHAIN", "2")
    part, lv, layout, op = _level(pm, n, P, None, coloured=True)
    assert op.chain_available() and op.chain_form()
    T = tr.rotating_tensor(_centres(part))
    op.set_coefficient_tensor(T)
    assert op.chain_form()
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    ref = _oracle(P, 2.0, part, lv, T).apply(u)
    chained = _apply(pm, op, layout, u).data_copy()
    assert _relerr(chained, ref) < 1e-12
    op.set_chain_form(False)
    assert _relerr(chained, _apply(pm, op, layout, u).data_copy()) < 1e-12


# ---- 7. fused residual restriction ------------------------------------------------------------------------------


def test_fused_residual_restriction(pm):
    from oracle import pmg_oracle as po

    pc, pf, n = 2, 4, (4, 4, 16)
    part = pm.BoxPartition(n, warp=warp)
    lc, lf = part.level(pc), part.level(pf)
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    fop = pm.MatFreeLaplacian(pf, 2.0, lf.dofmap, part.xgeom, part.geom_dofmap, lf.lcells, lf.bcells, lf.bc_marker, Lf)
    T = tr.random_spd(part.ncells, 7)
    fop.set_coefficient_tensor(T)
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    A = _oracle(pf, 2.0, part, lf, T)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    rng = np.random.default_rng(24)
    zu, ru = rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)
    z, r, q, coarse = _vec(pm, Lf, zu), _vec(pm, Lf, ru), pm.Vector(Lf), pm.Vector(Lc)
    coarse.set(3.0)
    ip.restrict_residual(fop, z, r, coarse)
    got = coarse.data_copy()
    assert _relerr(got, oi.reverse_interpolate(ru - A.apply(zu))) < 1e-12
    fop(z, q)
    d = pm.Vector(Lf)
    d.data.copy_(r.data - q.data)
    c2 = pm.Vector(Lc)
    ip.reverse_interpolate(d, c2)
    assert _relerr(got, c2.data_copy()) < 1e-12


# ---- 8. lifting -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_field", [False, True])
def test_lifting_follows_the_tensor(pm, with_field):
    P, n, alpha = 3, (3, 2, 4), 0.7
    part, lv, layout, op = _level(pm, n, P, twist)
    T = tr.random_spd(part.ncells, 80)
    kq = random_field(lv.ndofs, 81) if with_field else None
    if with_field:
        op.set_coefficient_field(_vec(pm, layout, kq))
    op.set_coefficient_tensor(T)
    rng = np.random.default_rng(82)
    g, x0, b0 = rng.standard_normal(lv.ndofs), rng.standard_normal(lv.ndofs), rng.standard_normal(lv.ndofs)
    marked = lv.bc_marker.astype(bool)
    Au = _oracle(P, 2.0, part, lv, T, kq, bc=np.zeros_like(lv.bc_marker))  # unconstrained
    ref = b0 - alpha * Au.apply(np.where(marked, g - x0, 0.0))
    b = _vec(pm, layout, b0)
    op.apply_lifting(_vec(pm, layout, g), b, x0=_vec(pm, layout, x0), alpha=alpha)
    got = b.data_copy()
    assert _relerr(got[~marked], ref[~marked]) < 1e-12
    assert np.array_equal(got[marked], b0[marked])
    plain = b0 - alpha * _oracle(P, 2.0, part, lv, bc=np.zeros_like(lv.bc_marker)).apply(np.where(marked, g - x0, 0.0))
    assert _relerr(plain[~marked], ref[~marked]) > 1e-2


# ---- 9. refusals ------------------------------------------------------------------------------------------------


BAD = {"zero": (0.0,) * 6, "indefinite": (1.0, 2.0, 0.0, 1.0, 0.0, 1.0), "negative zz": (1.0, 0.0, 0.0, 1.0, 0.0, -1.0),
       "nan": (1.0, 0.0, float("nan"), 1.0, 0.0, 1.0), "inf": (1.0, 0.0, 0.0, float("inf"), 0.0, 1.0)}


@pytest.mark.parametrize("with_tensor", [False, True])
def test_invalid_tensors_are_refused(pm, with_tensor):
    P, n = 2, (3, 2, 4)
    part, lv, layout, op = _level(pm, n, P, twist, coloured=True)
    good = tr.random_spd(part.ncells, 61)
    if with_tensor:
        op.set_coefficient_tensor(good)
    op.compute_diag_inverse()
    u = np.random.default_rng(6).standard_normal(lv.ndofs)
    before = _apply(pm, op, layout, u).data.clone()
    g_before, d_before = op.geometry().clone(), _diag(pm, op, layout)
    for i, (name, value) in enumerate(BAD.items()):
        bad = good.copy()
        bad[(5 * i + 3) % part.ncells] = value
        with pytest.raises(pm._lib.PmgError, match="1 cells have a tensor that is not finite and positive") as e:
            op.set_coefficient_tensor(bad)
        assert "(code -1)" in str(e.value), name  # PMG_ERR_INVALID
        assert op.has_coefficient_tensor() == with_tensor
        assert torch.equal(op.geometry(), g_before)
        assert np.array_equal(_diag(pm, op, layout), d_before)
        assert _relerr(_apply(pm, op, layout, u).data_copy(), before.cpu().numpy()) < NOISE
    # shape and dtype, from Python
    with pytest.raises(ValueError, match="shape"):
        op.set_coefficient_tensor(good[:-1])
    with pytest.raises(ValueError, match="shape"):
        op.set_coefficient_tensor(good.ravel())
    with pytest.raises(TypeError):
        op.set_coefficient_tensor(good.astype(np.float32))
    with pytest.raises(TypeError):
        op.set_coefficient_tensor(torch.from_numpy(good).cuda().float())
    with pytest.raises(TypeError):
        op.set_coefficient_tensor([list(r) for r in good])
    # inside a stream capture (the pattern of tests/test_gpu_boundary_data.py: the capture holds one kernel of its own
    # and the refused call, and is thrown away)
    from pmg_dolfinx_amd._lib import current_stream, lib, ptr

    dev = torch.from_numpy(good).cuda()
    side, scratch = torch.cuda.Stream(), torch.zeros(8, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc = lib().pmg_laplacian_set_coefficient_tensor(op.handle, ptr(dev), current_stream())
            msg = lib().pmg_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == -1 and b"pmg_laplacian_set_coefficient_tensor" in msg and b"stream capture" in msg
    torch.cuda.synchronize()
    assert op.has_coefficient_tensor() == with_tensor and torch.equal(op.geometry(), g_before)


# ---- 10. FP32 ---------------------------------------------------------------------------------------------------


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
    without a tensor, times 2 (the field test's reasoning: the tensor adds a few roundings per point, in double before
    the one rounding to float, and random_spd has a 4:1 range against the field's 5:1)."""
    n = (4, 4, 8)
    part, lv, layout, plain = _level(pm, n, P, twist)
    u32 = np.random.default_rng(70 + P).standard_normal(lv.ndofs).astype(np.float32)
    e0, y_plain = _fp32_vs_fp64(pm, plain, layout, u32)
    assert 0 < e0 < 1e-5
    T = tr.random_spd(part.ncells, 90 + P)
    _, _, _, early = _level(pm, n, P, twist)
    early.set_coefficient_tensor(T)  # before the first FP32 use
    e1, y_t = _fp32_vs_fp64(pm, early, layout, u32)
    plain.set_coefficient_tensor(T)  # the float tensor exists already
    e2, y_late = _fp32_vs_fp64(pm, plain, layout, u32)
    plain.set_coefficient_tensor(None)
    e3, y_again = _fp32_vs_fp64(pm, plain, layout, u32)
    print(f"P = {P}: fp32 vs fp64 without a tensor {e0:.3e}; tensor set first {e1:.3e}, set after FP32 use {e2:.3e}, "
          f"cleared {e3:.3e}")
    assert _relerr(y_t, y_plain) > 1e-2  # (the FP64 side has the tensor)
    assert e1 <= 2 * e0
    assert _relerr(y_late, y_t) < 1e-13 and e2 <= 2 * e0
    assert _relerr(y_again, y_plain) < 1e-13 and e3 <= 2 * e0


# ---- 11. assembled operator -------------------------------------------------------------------------------------


def test_assembled_operator_follows_the_tensor(pm):
    P, n = 3, (3, 2, 2)
    part, lv, layout, op = _level(pm, n, P, twist)
    T = tr.rotating_tensor(_centres(part))
    op.set_coefficient_tensor(T)
    M = pm.MatrixOperator(op)
    ref = _oracle(P, 2.0, part, lv, T).assemble_csr()
    assert abs(M.to_scipy() - ref).max() < 1e-12 * abs(ref).max()
    T2 = tr.random_spd(part.ncells, 81)
    op.set_coefficient_tensor(T2)
    assert abs(M.to_scipy() - ref).max() < 1e-12 * abs(ref).max()  # the matrix holds the values it was assembled with
    M.update_values()
    ref2 = _oracle(P, 2.0, part, lv, T2).assemble_csr()
    assert abs(M.to_scipy() - ref2).max() < 1e-12 * abs(ref2).max()
    assert abs(ref2 - ref).max() > 1e-2 * abs(ref).max()
    u = np.random.default_rng(82).standard_normal(lv.ndofs)
    ym, yf = pm.Vector(layout), _apply(pm, op, layout, u)
    M(_vec(pm, layout, u), ym)
    assert _relerr(ym.data_copy(), yf.data_copy()) < 1e-12


# ---- 12. cycle and solve ----------------------------------------------------------------------------------------


def _oracle_hierarchy(n, orders, k, kappa, wf, tensor):
    """The oracle's V-cycle on operators with the tensor, with their own eigenvalue estimates."""
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh(n, warp=wf)
    T = tensor(tr.cell_centres(mesh.xgeom, mesh.geom_dofmap))
    ops, sm, eigs = [], [], []
    for P in orders:
        A = tr.with_tensor(tr.laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap,
                                        mesh.boundary_marker(P)), T)
        ops.append(A)
        rng, _ = po.estimate_eig_range(A, A.ndofs)
        eigs.append(rng)
        sm.append(po.Chebyshev(rng, k))
    it = [po.Interpolator(orders[i], orders[i + 1], ops[i].dofmap, ops[i + 1].dofmap, ops[i].ndofs, ops[i + 1].ndofs)
          for i in range(len(orders) - 1)]
    return mesh, ops, po.MultigridPreconditioner(ops, sm, it, mesh.boundary_marker(orders[0])), eigs


def test_vcycle_pcg_and_graph(pm):
    from oracle import pmg_oracle as po

    n, orders, k = 4, (1, 2, 4), 3
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=k, warp=warp, kappa_tensor=tr.rotating_tensor)
    assert all(op.has_coefficient_tensor() for op in h.operators)
    mesh, ops, mg, eigs = _oracle_hierarchy(n, orders, k, 2.0, warp, tr.rotating_tensor)
    for got, ref in zip(h.eig_ranges, eigs):
        assert abs(got[1] - ref[1]) < 1e-8 * ref[1]
    b = h.rhs[-1].data_copy()
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)
    err = _relerr(x.data_copy(), mg.apply(b, np.zeros_like(b)))
    print(f"V-cycle with a coefficient tensor vs oracle: {err:.3e}")
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
    print(f"PCG iterations with a coefficient tensor: {its}, oracle {oits}")
    assert abs(its - oits) <= 1 and oits < 50
    r = pm.Vector(h.layouts[-1])
    h.operators[-1](xs, r)
    pm.axpy(r, -1.0, r, h.rhs[-1])
    assert pm.norm(r) < 1e-6 * pm.norm(h.rhs[-1])
    # a captured cycle stays valid over a second set_coefficient_tensor with other values: the buffers keep their
    # addresses.  (The smoothers keep their eigenvalue bounds; the eager cycle it is compared with does too.)

    def cycle():
        v = h.new_vector()
        v.set(0.0)
        h.mg.apply(h.rhs[-1], v)
        return v.data_copy()

    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    first = cycle()
    assert h.mg.graph_replays() == n0 + 1 and _relerr(first, x.data_copy()) < 1e-10
    centres = _centres(h.part)
    T2 = tr.rotating_tensor(centres[:, [2, 0, 1]])
    for op in h.operators:
        op.set_coefficient_tensor(T2)
    replayed = cycle()
    assert h.mg.graph_replays() == n0 + 2
    h.mg.set_graph(False)
    eager = cycle()
    assert _relerr(replayed, eager) < 1e-10
    assert _relerr(first, eager) > 1e-3  # the second tensor is another operator


# ---- 13. AMG coarse level ---------------------------------------------------------------------------------------


def test_amg_coarse_level_reads_the_tensor(pm):
    """The AMG set-up reads the tensor through the assembled level-0 matrix, and PCG with the p-multigrid cycle over
    the AMG coarse solve reaches rtol 1e-8 in fewer than 50 iterations: 10 on an MI355X (n = 6, orders (1, 2),
    warped mesh, rotating tensor); the count is printed."""
    n, orders = 6, (1, 2)
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=2, warp=warp, kappa_tensor=tr.rotating_tensor)
    amg = pm.AmgSolver(h.operators[0], cycles=1)
    mesh, ops, mg, eigs = _oracle_hierarchy(n, orders, 2, 2.0, warp, tr.rotating_tensor)
    ref = ops[0].assemble_csr()
    free = ~mesh.boundary_marker(1).astype(bool)
    A0 = amg.export(0, "A")
    assert abs(A0[free] - ref[free]).max() < 1e-12 * abs(ref).max()
    h.mg.set_coarse_solver(amg)
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(50)
    cg.set_tolerance(1e-8)
    xs = h.new_vector()
    xs.set(0.0)
    its = cg.solve(h.operators[-1], xs, h.rhs[-1], preconditioner=h.mg)
    h.mg.set_coarse_solver(None)
    print(f"PCG iterations with the AMG coarse solver and a coefficient tensor: {its}")
    r = pm.Vector(h.layouts[-1])
    h.operators[-1](xs, r)
    pm.axpy(r, -1.0, r, h.rhs[-1])
    assert its < 50 and pm.norm(r) < 1e-6 * pm.norm(h.rhs[-1])


# ---- 14. two ranks on one GPU -----------------------------------------------------------------------------------


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, args, timeout=120):
    """tests/test_gpu_coefficient_field.py's launcher: `world` spawned processes report (rank, result) or
    (rank, traceback); on the first failure, a dead rank or the time limit every process is terminated and joined --
    nothing further is started on the GPU."""
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
        lv, layout, op, part = H.levels[0], H.layouts[0], H.operators[0], H.part
        gm = po.BoxMesh(n, warp=warp)
        Tg = tr.random_spd(gm.ncells, 111)  # global, by global cell number (x slowest)
        A = tr.with_tensor(tr.laplacian(P, 2.0, gm.dofmap(P), gm.xgeom, gm.geom_dofmap, gm.boundary_marker(P)), Tg)
        cc = part.cell_coords
        mine = Tg[(cc[:, 0] * n[1] + cc[:, 1]) * n[2] + cc[:, 2]]  # owned cells, then ghost cells
        # one rank hands in a bad tensor (on an owned cell): both refuse, nothing changes
        bad = mine.copy()
        if rank == 1:
            bad[0] = (1.0, 2.0, 0.0, 1.0, 0.0, 1.0)
        refused = False
        try:
            op.set_coefficient_tensor(bad)
        except pm._lib.PmgError as e:
            refused = "(code -1)" in str(e)
        still_plain = not op.has_coefficient_tensor()
        op.set_coefficient_tensor(mine)  # the hierarchy computed the diagonal: it follows
        own = lv.local_to_global[: lv.size_local]
        ug = np.random.default_rng(11).standard_normal(A.ndofs)
        xl = np.zeros(lv.ndofs)
        xl[: lv.size_local] = ug[own]
        x, y, d = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
        x.data.copy_(torch.from_numpy(xl))
        op(x, y)
        op.get_diag_inverse(d)
        ref, dref = A.apply(ug)[own], A.diag_inverse()[own]
        dist.barrier()
        return {"ghost_cells": int(part.ncells - part.ncells_owned), "refused": refused, "still_plain": still_plain,
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


def test_two_ranks(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks(_rank_worker, 2, ((3, 4, 8), (1, 1, 2), 2))
    for out in res:
        assert out["ghost_cells"] > 0
        assert out["refused"] and out["still_plain"], out
        assert out["apply"] < 1e-12 and out["diag"] < 1e-12, out
