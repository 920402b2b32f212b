"""The reaction term (pmg_laplacian_set_reaction): -div(K grad u) + sigma u with sigma >= 0 constant per cell,
y = A x + d x on unmarked rows and y = x on marked ones.

The CPU truth is tests/reaction_reference.py -- the oracle's operator plus the vector d, pinned from first principles
in tests/test_reaction_abi.py.  sigma is random in [0, 4] per cell with about a fifth of the cells exactly 0
(``rr.random_sigma``).

How the errors are measured.  The term lives on the unmarked rows, and there it is small beside the stiffness part: d
is sigma times a lumped mass of order h^3 / P^3, the diagonal of A of order kappa h P.  A random vector has entries of
order 3 on the marked rows (y = x), so max|a - b| / max|b| over the whole vector would hide an unmarked row's error
behind them and could never see sigma <= 4 at the 1e-2 level (at P = 8 even with kappa -> 0).  So ``_rows`` asks MORE
than that measure: the marked rows must equal x exactly, and the relative max error is taken over the unmarked rows
alone, < 1e-12 in FP64 (two summation orders of the reference differ by 3e-16 there); and the per-cell kappa is drawn
from [0.5, 1.5] * 0.5 / P^2 (``_kappa``), which puts the term at several per cent to tens of per cent of an unmarked
row, so that "the unshifted reference is more than 1e-2 away" holds on those rows at every degree.  1e-10 after a
V-cycle and NOISE = 1e-14 for two applications on the same bits are the figures of
tests/test_gpu_coefficient_tensor.py."""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NOISE = 1e-14
SHEAR = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])
FULL_PATCHES = [(1, (8, 8, 16)), (2, (4, 4, 16)), (3, (4, 4, 8)), (4, (4, 4, 8)), (5, (4, 4, 14)), (6, (2, 4, 8)),
                (7, (2, 2, 6)), (8, (2, 2, 6))]


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


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _rows(got, ref, x, bc):
    """Marked rows: y = x exactly (asserted).  Returns the relative max error over the unmarked rows."""
    marked = np.asarray(bc).astype(bool)
    assert np.array_equal(got[marked], np.asarray(x)[marked])
    return _relerr(got[~marked], ref[~marked])


def _kappa(P, ncells, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, ncells) * 0.5 / P**2


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _level(pm, n, P, wf, kappa, coloured=False, bc=None):
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


def _case(pm, n, P, wf, seed, coloured=False, bc=None):
    """(part, lv, layout, op, kappa, sigma, bc): an operator without the term yet, and the test's coefficients."""
    ncells = pm.BoxPartition(n, warp=wf).ncells
    kappa = _kappa(P, ncells, 300 + seed)
    part, lv, layout, op = _level(pm, n, P, wf, kappa, coloured, bc)
    return part, lv, layout, op, kappa, rr.random_sigma(ncells, 500 + seed), lv.bc_marker if bc is None else bc


def _oracle(P, kappa, sigma, part, lv, bc=None):
    return rr.laplacian(P, kappa, sigma, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker if bc is None else bc)


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


# ---- 1. every degree, both output forms -------------------------------------------------------------------------


@pytest.mark.parametrize("coloured", [False, True], ids=["default-plan", "coloured-stores"])
@pytest.mark.parametrize("P", range(1, 9))
def test_apply_and_diagonal_all_degrees(pm, P, coloured):
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, P, coloured)
    assert not op.has_reaction()
    op.set_reaction(sigma)
    assert op.has_reaction()
    A = _oracle(P, kappa, sigma, part, lv)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    ref = A.apply(u)
    err = _rows(_apply(pm, op, layout, u).data_copy(), ref, u, bc)
    op.compute_diag_inverse()
    derr = _relerr(_diag(pm, op, layout), A.diag_inverse())
    away = _rows(A.A.apply(u), ref, u, bc)
    print(f"P = {P} {'coloured' if coloured else 'default'}: apply {err:.3e}, inverse diagonal {derr:.3e}; "
          f"the operator without the term is {away:.3e} away")
    assert err < 1e-12
    assert derr < 1e-12
    assert away > 1e-2
    # a device tensor is taken as it is
    op.set_reaction(torch.from_numpy(sigma).cuda())
    assert _rows(_apply(pm, op, layout, u).data_copy(), ref, u, bc) < 1e-12


# ---- 2. full patches --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P,n", FULL_PATCHES)
def test_apply_full_patches(pm, P, n):
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, None, 20 + P)
    op.set_reaction(sigma)
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    ref = _oracle(P, kappa, sigma, part, lv).apply(u)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(-3.0)
    op(x, y)
    assert _rows(y.data_copy(), ref, u, bc) < 1e-12
    op(x, y)  # second application into the same y: no dependence on its previous content
    assert _rows(y.data_copy(), ref, u, bc) < 1e-12


# ---- 3. a marker with interior marked dofs ----------------------------------------------------------------------


@pytest.mark.parametrize("P,n,coloured", [(2, (5, 4, 3), False), (4, (4, 4, 8), True), (5, (3, 2, 4), False)])
def test_interior_marked_dofs(pm, P, n, coloured):
    lv0 = pm.BoxPartition(n, warp=twist).level(P)
    extra = np.random.default_rng(40 + P).uniform(size=lv0.ndofs) < 0.1
    bc = (lv0.bc_marker.astype(bool) | extra).astype(np.int8)
    assert bc.sum() > lv0.bc_marker.sum() + 5
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 40 + P, coloured, bc=bc)
    op.set_reaction(sigma)
    A = _oracle(P, kappa, sigma, part, lv, bc)
    u = np.random.default_rng(41 + P).standard_normal(lv.ndofs)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12  # marked rows: y = x exactly
    op.compute_diag_inverse()
    dinv = _diag(pm, op, layout)
    assert np.array_equal(dinv[bc.astype(bool)], np.ones(int(bc.sum())))
    assert _relerr(dinv, A.diag_inverse()) < 1e-12


# ---- 4. set, change, clear --------------------------------------------------------------------------------------


def test_set_change_clear(pm):
    P, n = 4, (4, 4, 8)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 3, coloured=True)
    u = np.random.default_rng(3).standard_normal(lv.ndofs)
    before = _apply(pm, op, layout, u).data_copy()
    op.compute_diag_inverse()
    d_before = _diag(pm, op, layout)
    for s in (sigma, rr.random_sigma(part.ncells, 77), np.zeros(part.ncells)):  # (all zeros is legal)
        op.set_reaction(s)
        assert op.has_reaction()
        A = _oracle(P, kappa, s, part, lv)
        assert _rows(_apply(pm, op, layout, u, fill=1.0).data_copy(), A.apply(u), u, bc) < 1e-12
        # the inverse diagonal has followed, without another compute_diag_inverse
        assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    op.set_reaction(None)
    assert not op.has_reaction()
    assert _relerr(_apply(pm, op, layout, u).data_copy(), before) < NOISE
    assert _relerr(_diag(pm, op, layout), d_before) < NOISE  # recomputed: its atomics arrive in any order
    op.set_reaction(None)  # nothing to remove: no error
    # a diagonal installed by the caller is not overwritten
    mine = np.random.default_rng(5).uniform(0.1, 1.0, lv.ndofs)
    op.set_diag_inverse(_vec(pm, layout, mine))
    op.set_reaction(sigma)
    assert np.array_equal(_diag(pm, op, layout), mine)
    op.set_reaction(None)
    assert np.array_equal(_diag(pm, op, layout), mine)


@pytest.mark.parametrize("P,n,coloured", [(4, (4, 4, 8), True), (2, (5, 4, 3), False)])
def test_clear_restores_apply_and_diagonal_bit_for_bit(pm, P, n, coloured):
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 3, coloured)
    _, _, _, fresh = _level(pm, n, P, twist, kappa, coloured)
    u = _order_free_vector(P, lv, 3)
    before = _apply(pm, fresh, layout, u).data.clone()
    assert torch.equal(_apply(pm, op, layout, u).data, before)  # the premise: this vector's apply is reproducible
    fresh.compute_diag_inverse()
    op.compute_diag_inverse()
    for s in (sigma, rr.random_sigma(part.ncells, 78)):
        op.set_reaction(s)
        assert not torch.equal(_apply(pm, op, layout, u).data, before)  # ... and it sees the term
    op.set_reaction(None)
    assert torch.equal(_apply(pm, op, layout, u).data, before)
    # the diagonal: against a fresh operator, whose sums met in whatever order (NOISE); with the order-free structure
    # out of reach there, bit identity is asserted where one cell alone holds the dof (a single addend)
    d_op, d_fresh = _diag(pm, op, layout), _diag(pm, fresh, layout)
    assert _relerr(d_op, d_fresh) < NOISE
    single = np.bincount(np.asarray(lv.dofmap).ravel(), minlength=lv.ndofs) == 1
    assert single.sum() > 0 and np.array_equal(d_op[single], d_fresh[single])
    # the FP32 form as well (single domain): built while the term was set, restored by the removal
    x32 = torch.from_numpy(u.astype(np.float32)).cuda()
    y_op, y_fresh = torch.full_like(x32, 7.0), torch.full_like(x32, 7.0)
    op.set_reaction(sigma)
    op.apply_fp32(x32, y_op)
    fresh.apply_fp32(x32, y_fresh)
    assert not torch.equal(y_op, y_fresh)
    op.set_reaction(None)
    op.apply_fp32(x32, y_op)
    assert torch.equal(y_op, y_fresh)


def test_invalid_input_is_refused(pm):
    P, n = 2, (3, 2, 4)
    for with_term in (False, True):
        part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 6, coloured=True)
        if with_term:
            op.set_reaction(sigma)
        op.compute_diag_inverse()
        u = np.random.default_rng(6).standard_normal(lv.ndofs)
        before, d_before = _apply(pm, op, layout, u).data_copy(), _diag(pm, op, layout)
        for i, value in enumerate((float("nan"), -1e-300, -2.0, float("inf"))):
            bad = sigma.copy()
            bad[(5 * i + 3) % part.ncells] = value
            with pytest.raises(pm._lib.PmgError, match="1 cells have a value that is not finite and >= 0") as e:
                op.set_reaction(bad)
            assert "(code -1)" in str(e.value)  # PMG_ERR_INVALID
            assert op.has_reaction() == with_term
            assert np.array_equal(_diag(pm, op, layout), d_before)
            assert _relerr(_apply(pm, op, layout, u).data_copy(), before) < NOISE
        bad = sigma.copy()
        bad[:3] = -1.0
        with pytest.raises(pm._lib.PmgError, match="3 cells"):
            op.set_reaction(bad)
        # shape and dtype, from Python
        with pytest.raises(ValueError, match="shape"):
            op.set_reaction(sigma[:-1])
        with pytest.raises(ValueError, match="shape"):
            op.set_reaction(sigma[:, None])
        with pytest.raises(TypeError):
            op.set_reaction(sigma.astype(np.float32))
        with pytest.raises(TypeError):
            op.set_reaction(list(sigma))
        # inside a stream capture (the pattern of tests/test_gpu_coefficient_tensor.py: the capture holds one kernel of
        # its own and the refused call, and is thrown away)
        from pmg_dolfinx_amd._lib import current_stream, lib, ptr

        dev = torch.from_numpy(sigma).cuda()
        side, scratch = torch.cuda.Stream(), torch.zeros(8, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                scratch.add_(1.0)
                rc = lib().pmg_laplacian_set_reaction(op.handle, ptr(dev), current_stream())
                msg = lib().pmg_last_error()
        torch.cuda.current_stream().wait_stream(side)
        assert rc == -1 and b"pmg_laplacian_set_reaction" in msg and b"stream capture" in msg
        torch.cuda.synchronize()
        assert op.has_reaction() == with_term
        assert np.array_equal(_diag(pm, op, layout), d_before)
        assert _relerr(_apply(pm, op, layout, u).data_copy(), before) < NOISE


# ---- 5. modes ---------------------------------------------------------------------------------------------------


def test_affine_mode(pm):
    P, n = 4, (4, 4, 8)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, None, 50)  # an unwarped box
    assert op.is_affine()
    op.set_reaction(sigma)
    u = np.random.default_rng(50).standard_normal(lv.ndofs)
    A = _oracle(P, kappa, sigma, part, lv)
    op.set_geometry_mode("affine")
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12
    sigma2 = rr.random_sigma(part.ncells, 51)  # set while in affine mode
    op.set_reaction(sigma2)
    A2 = _oracle(P, kappa, sigma2, part, lv)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A2.apply(u), u, bc) < 1e-12
    op.set_geometry_mode("stored")
    assert _rows(_apply(pm, op, layout, u).data_copy(), A2.apply(u), u, bc) < 1e-12


@pytest.mark.parametrize("term_first", [True, False])
def test_batched_geometry(pm, term_first):
    from pmg_dolfinx_amd import _lib

    P, n = 2, (4, 4, 16)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 52, coloured=True)
    if term_first:
        op.set_reaction(sigma)
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 8)  # the Python class refuses batching: the C entry point
    if not term_first:
        op.set_reaction(sigma)
    A = _oracle(P, kappa, sigma, part, lv)
    u = np.random.default_rng(8).standard_normal(lv.ndofs)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12
    op.compute_diag_inverse()
    assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)  # back to the resident tensor: the term is still there
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12


def test_chain_form_requested(pm, monkeypatch):
    """The chain kernel does not carry the term: while one is set, an operator in chain form runs its interior as the
    column launches (and says so in launches_per_apply); the chains come back with the removal.  (4, 4, 64) is the
    shape of tests/test_gpu_coefficient_tensor.py::test_chain_form: sixteen 2 x 2 x 8 patches in a row, the smallest
    on which chains exist."""
    P, n = 4, (4, 4, 64)
    monkeypatch.setenv("PMG_CHAIN", "2")
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, None, 53, coloured=True)
    assert op.chain_available() and op.chain_form()
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    chained = op.launches_per_apply()
    plain = _apply(pm, op, layout, u).data_copy()  # through the chain kernel
    op.set_chain_form(False)
    columns = op.launches_per_apply()
    assert _relerr(_apply(pm, op, layout, u).data_copy(), plain) < 1e-12
    op.set_chain_form(True)
    print(f"launches per apply: {chained} as chains, {columns} as columns")
    assert chained != columns and op.launches_per_apply() == chained
    op.set_reaction(sigma)
    assert op.chain_form()  # still requested ...
    assert op.launches_per_apply() == columns  # ... and bypassed
    A = _oracle(P, kappa, sigma, part, lv)
    op.set_profiling(True)  # (the profile counts the kernel launches of the application below)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12
    assert op.read_profile()[1] == columns
    op.set_profiling(False)
    # an apply that dropped the term would be this far off: on this mesh the cells are 1/4 x 1/4 x 1/64, the stiffness
    # part grows with 1 / h_z and the term is a few 1e-4 of a row (a property of the reference alone, computed on the
    # host) -- what matters is that it is many orders above the 1e-12 just asserted
    assert _rows(A.A.apply(u), A.apply(u), u, bc) > 1e-6
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    assert op.time_kernel(x, y, 2) > 0  # divides by launches_per_apply
    op.set_reaction(None)
    assert op.chain_form() and op.launches_per_apply() == chained
    assert _relerr(_apply(pm, op, layout, u).data_copy(), plain) < NOISE


def test_chain_form_unavailable(pm, monkeypatch):
    """(4, 4, 8): four patches, too few for a chain.  The request is refused with or without the term, and the apply
    with the term is the column launches'."""
    P, n = 4, (4, 4, 8)
    monkeypatch.setenv("PMG_CHAIN", "2")
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, None, 53, coloured=True)
    assert not op.chain_available()
    op.set_reaction(sigma)
    with pytest.raises(pm._lib.PmgError, match="no chains"):
        op.set_chain_form(True)
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    assert _rows(_apply(pm, op, layout, u).data_copy(), _oracle(P, kappa, sigma, part, lv).apply(u), u, bc) < 1e-12


def test_with_nodal_field_and_tensor(pm):
    P, n = 3, (3, 2, 4)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 54)
    T = tr.random_spd(part.ncells, 55)
    kq = np.random.default_rng(56).uniform(0.5, 2.0, lv.ndofs)
    op.set_reaction(sigma)  # first: the term does not depend on the stored tensor
    op.set_coefficient_field(_vec(pm, layout, kq))
    op.set_coefficient_tensor(T)
    assert op.has_reaction() and op.has_coefficient_field() and op.has_coefficient_tensor()
    D = tr.with_tensor(tr.laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker), T, kq)
    A = rr.ReactionLaplacian(D, sigma, part.xgeom, part.geom_dofmap)
    u = np.random.default_rng(57).standard_normal(lv.ndofs)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A.apply(u), u, bc) < 1e-12
    op.compute_diag_inverse()
    assert _relerr(_diag(pm, op, layout), A.diag_inverse()) < 1e-12
    op.set_coefficient_tensor(None)
    op.set_coefficient_field(None)
    A0 = _oracle(P, kappa, sigma, part, lv)
    assert _rows(_apply(pm, op, layout, u).data_copy(), A0.apply(u), u, bc) < 1e-12
    assert _relerr(_diag(pm, op, layout), A0.diag_inverse()) < 1e-12


# ---- 6. FP32 ----------------------------------------------------------------------------------------------------


def _fp32_vs_fp64(pm, op, layout, u32, bc):
    x = torch.from_numpy(u32).cuda()
    y = torch.full_like(x, 7.0)
    op.apply_fp32(x, y)
    torch.cuda.synchronize()
    ref = _apply(pm, op, layout, u32.astype(np.float64)).data_copy()
    return _rows(y.cpu().numpy().astype(np.float64), ref, u32.astype(np.float64), bc), ref


@pytest.mark.parametrize("P", [4, 1])
def test_fp32_apply(pm, P):
    """apply_fp32 against the FP64 apply of the same operator.  The bound is that of
    tests/test_gpu_coefficient_tensor.py: the same error measured on the same mesh without the term, times 2 (the term
    adds one rounding of d to float and one product per dof, beside the few hundred of the stiffness part)."""
    n = (4, 4, 8)
    part, lv, layout, plain, kappa, sigma, bc = _case(pm, n, P, twist, 70 + P)
    u32 = np.random.default_rng(70 + P).standard_normal(lv.ndofs).astype(np.float32)
    e0, y_plain = _fp32_vs_fp64(pm, plain, layout, u32, bc)
    assert 0 < e0 < 1e-5
    _, _, _, early = _level(pm, n, P, twist, kappa)
    early.set_reaction(sigma)  # before the first FP32 use
    e1, y_t = _fp32_vs_fp64(pm, early, layout, u32, bc)
    plain.set_reaction(sigma)  # the float tensor exists already
    e2, y_late = _fp32_vs_fp64(pm, plain, layout, u32, bc)
    plain.set_reaction(None)
    e3, y_again = _fp32_vs_fp64(pm, plain, layout, u32, bc)
    print(f"P = {P}: fp32 vs fp64 without the term {e0:.3e}; term set first {e1:.3e}, set after FP32 use {e2:.3e}, "
          f"cleared {e3:.3e}")
    free = ~np.asarray(bc).astype(bool)
    assert _relerr(y_t[free], y_plain[free]) > 1e-2  # (the FP64 side has the term)
    assert e1 <= 2 * e0
    assert _relerr(y_late, y_t) < 1e-13 and e2 <= 2 * e0
    assert _relerr(y_again, y_plain) < 1e-13 and e3 <= 2 * e0


# ---- 7. fused residual restriction ------------------------------------------------------------------------------


@pytest.mark.parametrize("pc,pf,n", [(1, 2, (4, 4, 16)), (2, 4, (4, 4, 16))])
def test_fused_residual_restriction(pm, pc, pf, n):
    from oracle import pmg_oracle as po

    part = pm.BoxPartition(n, warp=warp)
    lc, lf = part.level(pc), part.level(pf)
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    kappa, sigma = _kappa(pf, part.ncells, 24), rr.random_sigma(part.ncells, 25)
    fop = pm.MatFreeLaplacian(pf, kappa, lf.dofmap, part.xgeom, part.geom_dofmap, lf.lcells, lf.bcells, lf.bc_marker,
                              Lf)
    fop.set_reaction(sigma)
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    A = _oracle(pf, kappa, sigma, part, lf)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    rng = np.random.default_rng(24)
    zu, ru = rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)
    z, r, coarse = _vec(pm, Lf, zu), _vec(pm, Lf, ru), pm.Vector(Lc)
    coarse.set(3.0)
    ip.restrict_residual(fop, z, r, coarse)
    got = coarse.data_copy()
    ref = oi.reverse_interpolate(ru - A.apply(zu))  # the explicitly formed r - (A + D) z
    without = oi.reverse_interpolate(ru - A.A.apply(zu))
    print(f"{pf} -> {pc}: fused restriction {_relerr(got, ref):.3e}; without the term {_relerr(without, ref):.3e} away")
    assert _relerr(got, ref) < 1e-12
    assert _relerr(without, ref) > 1e-4  # (r is of order 1 on every row, the term a small part of A z: eight orders above the bound)


def test_vcycle_fused_against_separate(pm):
    n, orders = 4, (1, 2, 4)
    h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=warp,
                            reaction=lambda c: rr.random_sigma(len(c), 26))
    assert all(op.has_reaction() for op in h.operators)

    def cycle():
        v = h.new_vector()
        v.set(0.0)
        h.mg.apply(h.rhs[-1], v)
        return v.data_copy()

    h.mg.set_fused_restriction(None)  # mode -1, the default route
    fused = cycle()
    assert h.mg.fused_restrictions() > 0
    h.mg.set_fused_restriction(0)
    separate = cycle()
    assert h.mg.fused_restrictions() == 0
    assert _relerr(fused, separate) < 1e-11
    # the cycle is that of the operator with the term: the oracle's V-cycle on the helper's operators
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh(n, warp=warp)
    sigma = rr.random_sigma(mesh.ncells, 26)
    ops = [rr.laplacian(P, 0.05, sigma, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P))
           for P in orders]
    sm = [po.Chebyshev(e, 3) for e in h.eig_ranges]  # the device run's bounds: only the cycle's arithmetic is compared
    it = [po.Interpolator(orders[i], orders[i + 1], ops[i].dofmap, ops[i + 1].dofmap, ops[i].ndofs, ops[i + 1].ndofs)
          for i in range(len(orders) - 1)]
    mg = po.MultigridPreconditioner(ops, sm, it, mesh.boundary_marker(orders[0]))
    b = h.rhs[-1].data_copy()
    assert _relerr(separate, mg.apply(b, np.zeros_like(b))) < 1e-10


# ---- 8. assembled operator --------------------------------------------------------------------------------------


def test_assembled_operator(pm):
    P, n = 2, (2, 2, 2)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, twist, 80)
    op.set_reaction(sigma)
    M = pm.MatrixOperator(op)
    ref = _oracle(P, kappa, sigma, part, lv).dense()
    assert np.abs(M.to_scipy().toarray() - ref).max() < 1e-13 * np.abs(ref).max()
    sigma2 = rr.random_sigma(part.ncells, 81)
    op.set_reaction(sigma2)
    assert np.abs(M.to_scipy().toarray() - ref).max() < 1e-13 * np.abs(ref).max()  # the values it was assembled with
    M.update_values()
    ref2 = _oracle(P, kappa, sigma2, part, lv).dense()
    assert np.abs(M.to_scipy().toarray() - ref2).max() < 1e-13 * np.abs(ref2).max()
    assert np.abs(ref2 - ref).max() > 1e-2 * np.abs(ref).max()
    u = np.random.default_rng(82).standard_normal(lv.ndofs)
    ym, yf = pm.Vector(layout), _apply(pm, op, layout, u)
    M(_vec(pm, layout, u), ym)
    assert _rows(ym.data_copy(), yf.data_copy(), u, bc) < 1e-12
    dm = pm.Vector(layout)
    M.get_diag_inverse(dm)
    assert _relerr(dm.data_copy(), _oracle(P, kappa, sigma2, part, lv).diag_inverse()) < 1e-12
    op.set_reaction(None)  # ... and a removal
    M.update_values()
    plain = _oracle(P, kappa, np.zeros(part.ncells), part, lv).dense()
    assert np.abs(M.to_scipy().toarray() - plain).max() < 1e-13 * np.abs(plain).max()


def test_cycle_with_an_assembled_level(pm):
    n, orders = 4, (1, 2)
    reaction = lambda c: rr.random_sigma(len(c), 83)  # noqa: E731
    h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=2, warp=warp, reaction=reaction, assembled_levels=(0,))

    def cycle(hh):
        v = hh.new_vector()
        v.set(0.0)
        hh.mg.apply(hh.rhs[-1], v)
        return v.data_copy()

    assembled = cycle(h)
    h.mg.set_level_matrix(0, None)
    matrix_free = cycle(h)
    assert _relerr(assembled, matrix_free) < 1e-10
    plain = cycle(pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=2, warp=warp, assembled_levels=(0,)))
    assert _relerr(plain, assembled) > 1e-3  # the matrix carries the term


# ---- 9. solve ---------------------------------------------------------------------------------------------------


def _pcg(pm, h, rtol=1e-10, max_iter=60):
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(max_iter)
    cg.set_tolerance(rtol)
    x = h.new_vector()
    x.set(0.0)
    its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
    return its, x.data_copy()


@pytest.fixture(scope="module")
def solve_reference():
    """The fine-level helper operators of the solve tests, by seed, built once."""
    from oracle import pmg_oracle as po

    mesh = po.BoxMesh((8, 8, 8))
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = rr.laplacian(4, 2.0, rr.random_sigma(mesh.ncells, seed), mesh.dofmap(4), mesh.xgeom,
                                       mesh.geom_dofmap, mesh.boundary_marker(4))
        return cache[seed]

    return get


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_solve_with_amg_pcg_and_graph(pm, precision, solve_reference):
    """PoissonHierarchy((8, 8, 8), (1, 2, 4), reaction=...) as it comes (kappa = 2, the unit cube), PCG to 1e-10.  CG
    stops on r . M^-1 r, so the 2-norm residual formed on the host sits a small factor above 1e-10: 2.9e-10 in the CPU
    oracle's PCG on this problem (coarsest level solved exactly), against the bound 1e-9."""
    n, orders = (8, 8, 8), (1, 2, 4)

    def hierarchy(reaction):
        h = pm.PoissonHierarchy(n, orders, reaction=reaction)
        h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], cycles=2))  # stationary: a fixed linear preconditioner
        h.mg.set_precision(precision)
        h.mg.set_graph(True)
        return h

    def residual(h, x, seed):
        b = h.rhs[-1].data_copy()
        return np.linalg.norm(b - solve_reference(seed).apply(x)) / np.linalg.norm(b)  # formed on the host

    h0 = hierarchy(None)
    its0, _ = _pcg(pm, h0)
    h = hierarchy(lambda c: rr.random_sigma(len(c), 90))
    assert all(op.has_reaction() for op in h.operators) and h.mg.precision == precision
    n0 = h.mg.graph_replays()
    its, x = _pcg(pm, h)
    res = residual(h, x, 90)
    print(f"{precision}: PCG iterations with the term {its}, without {its0}; host residual {res:.3e}, "
          f"graph replays {h.mg.graph_replays() - n0}")
    assert h.mg.graph_replays() > n0
    assert res < 1e-9
    assert its <= its0 + 2
    # a second set with other values: the cached graph is replayed on the rewritten vectors (FP32: re-captured, its
    # float diagonal changed); the AMG hierarchy and the eigenvalue bounds stay the first set's, the caller's to renew
    sigma2 = rr.random_sigma(h.part.ncells, 91)
    for op in h.operators:
        op.set_reaction(sigma2)
    n1 = h.mg.graph_replays()
    its2, x2 = _pcg(pm, h)
    res2 = residual(h, x2, 91)
    print(f"{precision}: after a second set: {its2} iterations, host residual {res2:.3e}")
    assert h.mg.graph_replays() > n1
    assert res2 < 1e-9
    assert residual(h, x2, 90) > 1e-6  # the second operator is another one


# ---- 10. AMG alone ----------------------------------------------------------------------------------------------


def test_amg_alone(pm):
    P, n = 1, (8, 8, 8)
    part, lv, layout, op, kappa, sigma, bc = _case(pm, n, P, warp, 95)
    op.set_reaction(sigma)
    op.compute_diag_inverse()
    A = _oracle(P, kappa, sigma, part, lv)
    amg = pm.AmgSolver(op, max_iter=60, rtol=1e-9)
    free = ~np.asarray(bc).astype(bool)
    d0 = amg.export(0, "A").diagonal()
    ref = A.diagonal()
    assert np.abs(d0 - ref)[free].max() < 1e-13 * np.abs(ref[free]).max()
    assert np.abs(d0 - A.A.diagonal())[free].max() > 1e-2 * np.abs(ref[free]).max()  # the term is on it
    bu = np.random.default_rng(96).standard_normal(lv.ndofs)
    bu[~free] = 0.0
    x, b = pm.Vector(layout), _vec(pm, layout, bu)
    x.set(0.0)
    its = amg.solve(x, b)
    res = np.linalg.norm(bu - A.apply(x.data_copy())) / np.linalg.norm(bu)
    print(f"pmg_amg_solve with the term: {its} iterations, host residual {res:.3e}")
    assert its < 60 and res < 1e-8


# ---- 11. two ranks on one GPU -----------------------------------------------------------------------------------


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, args, timeout=120):
    """tests/test_gpu_coefficient_tensor.py's launcher: `world` spawned processes report (rank, result) or
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


def _rank_body(rank, world, port, n, dims, degrees):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm
        from oracle import pmg_oracle as po

        torch.cuda.set_device(0)
        out = {}
        for P in degrees:
            kap = 0.5 / P**2
            H = pm.PoissonHierarchy(n, (P,), kappa=kap, proc_dims=dims, rank=rank, size=world, warp=warp)
            lv, layout, op, part = H.levels[0], H.layouts[0], H.operators[0], H.part
            gm = po.BoxMesh(n, warp=warp)
            sg = rr.random_sigma(gm.ncells, 111)  # global, by global cell number (x slowest)
            A = rr.laplacian(P, kap, sg, gm.dofmap(P), gm.xgeom, gm.geom_dofmap, gm.boundary_marker(P))
            cc = part.cell_coords
            mine = sg[(cc[:, 0] * n[1] + cc[:, 1]) * n[2] + cc[:, 2]]  # owned cells, then ghost cells
            # one rank hands in a bad value (on an owned cell): both refuse, nothing changes
            bad = mine.copy()
            if rank == 1:
                bad[0] = -1.0
            refused = False
            try:
                op.set_reaction(bad)
            except pm._lib.PmgError as e:
                refused = "(code -1)" in str(e)
            still_plain = not op.has_reaction()
            op.set_reaction(mine)  # the hierarchy computed the diagonal: it follows
            own = lv.local_to_global[: lv.size_local]
            ug = np.random.default_rng(11).standard_normal(A.ndofs)
            xl = np.zeros(lv.ndofs)
            xl[: lv.size_local] = ug[own]
            x, y, d = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
            x.data.copy_(torch.from_numpy(xl))
            op(x, y)
            op.get_diag_inverse(d)
            ref, dref, plain = A.apply(ug)[own], A.diag_inverse()[own], A.A.apply(ug)[own]
            free = ~gm.boundary_marker(P).astype(bool)[own]
            got = y.data_copy()[: lv.size_local]
            dist.barrier()
            out[P] = {"ghost_cells": int(part.ncells - part.ncells_owned), "refused": refused,
                      "still_plain": still_plain,
                      "marked_exact": bool(np.array_equal(got[~free], ug[own][~free])),
                      "apply": float(np.abs(got - ref)[free].max() / np.abs(ref[free]).max()),
                      "away": float(np.abs(plain - ref)[free].max() / np.abs(ref[free]).max()),
                      "diag": float(np.abs(d.data_copy()[: lv.size_local] - dref).max() / np.abs(dref).max())}
        return out
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
    res = _run_ranks(_rank_worker, 2, ((3, 4, 8), (1, 1, 2), (2, 4)))
    for per_rank in res:
        for P, out in per_rank.items():
            assert out["ghost_cells"] > 0
            assert out["refused"] and out["still_plain"], (P, out)
            assert out["marked_exact"], (P, out)
            assert out["apply"] < 1e-12 and out["diag"] < 1e-12, (P, out)
            assert out["away"] > 1e-2, (P, out)
