"""The recomputed tensor of the low-degree apply (pmg_laplacian_set_tensor_recompute; TensorStream's GEO_RECOMPUTE
form in pmg-dolfinx_amd/csrc/stiffness_layer.hpp): the column and the fused restrict kernel with the form on and off,
against the oracle and against each other; V-cycles, eager and replayed; and every configuration in which an operator
must keep streaming G.

Bounds: 1e-12 of max |y| for one application or transfer, 1e-10 after V-cycles (as
tests/test_gpu_parity.py and tests/test_gpu_fused_restriction.py); NOISE = 1e-14 for the same kernels on the same bits
twice (LDS and global atomics arrive in any order; tests/test_gpu_reaction.py).  The two forms differ by rounding of
G alone; the largest difference seen is printed (about 1e-15) and held to the 1e-12 bar.

Degrees: the form is instantiated, and the automatic choice, at P = 1 and P = 2 (profiles/tensor_recompute.md)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL, TOL_CYCLE, NOISE = 1e-12, 1e-10, 1e-14
FORM_DEGREES = (1, 2)  # degrees whose kernels have the form (recompute_form, laplacian.hip)
AUTO_DEGREES = (1, 2)  # ... and where it is the automatic choice (recompute_default)
OBSERVED = {"forms": 0.0}
SHEAR = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])


def shear(x):
    return x @ SHEAR.T


def jitter(n):
    """Every interior vertex moved by up to 0.2 h along each axis, by a fixed function of its position (the oracle's
    mesh and the library's are built separately): non-affine trilinear cells, no tensor grid of centroids."""
    h = 1.0 / np.asarray(n, dtype=np.float64)

    def f(x):
        d = 0.2 * h * np.sin(37.0 * x[:, [1, 2, 0]] + 91.0 * x + np.array([1.0, 2.0, 3.0]))
        inside = np.all((x > 1e-9) & (x < 1.0 - 1e-9), axis=1)
        return x + d * inside[:, None]

    return f


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


def _apply(pm, op, layout, u, fill=7.0):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(fill)
    op(x, y)
    return y.data_copy()


_PARTS = {}


def _part(pm, mesh):
    """jitter: 5 x 6 x 17, patches cut short on all three axes, Morton patches; shear: one full patch of affine cells;
    frames: the 48 cell-local frames, once each, on twisted cells (the builder of tests/test_gpu_cell_frames.py)."""
    if mesh not in _PARTS:
        if mesh == "jitter":
            n = (5, 6, 17)
            _PARTS[mesh] = pm.BoxPartition(n, warp=jitter(n))
        elif mesh == "shear":
            _PARTS[mesh] = pm.BoxPartition((4, 4, 16), warp=shear)
        else:
            from test_gpu_cell_frames import MAPS, N48, frames_for

            _PARTS[mesh] = pm.BoxPartition(N48, warp=MAPS["twist"], cell_frames=frames_for(pm, N48, "mixed"))
    return _PARTS[mesh]


def _kappa(ncells):
    return np.random.default_rng(3).uniform(0.5, 2.0, ncells)


def _operator(pm, part, P, bc, coloured=False, **kw):
    lv = part.level(P)
    layout = pm.make_layout(lv)
    try:
        pm.set_merge_threshold(0 if coloured else -1)
        op = pm.MatFreeLaplacian(P, _kappa(part.ncells), lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                 bc, layout, **kw)
    finally:
        pm.set_merge_threshold(-1)
    return lv, layout, op


_REFS = {}


def _reference(part, mesh, P, markers, reaction):
    """The oracle's A u (+ d u), computed once per case and shared by the launch plans."""
    key = (mesh, P, markers, reaction)
    if key not in _REFS:
        lv = part.level(P)
        bc = lv.bc_marker if markers else np.zeros_like(lv.bc_marker)
        sigma = rr.random_sigma(part.ncells, 11) if reaction else np.zeros(part.ncells)
        A = rr.laplacian(P, _kappa(part.ncells), sigma, lv.dofmap, part.xgeom, part.geom_dofmap, bc)
        u = np.random.default_rng(7 + P).standard_normal(lv.ndofs)
        _REFS[key] = (bc, sigma, u, A.apply(u))
    return _REFS[key]


@pytest.mark.parametrize("reaction", [False, True])
@pytest.mark.parametrize("markers", [True, False])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("mesh", ["jitter", "shear", "frames"])
def test_apply_recomputed_against_stream_and_oracle(pm, mesh, P, markers, reaction):
    from pmg_dolfinx_amd import _lib

    part = _part(pm, mesh)
    bc, sigma, u, ref = _reference(part, mesh, P, markers, reaction)
    for coloured in (True, False):
        lv, layout, op = _operator(pm, part, P, bc, coloured)
        if mesh == "jitter":  # (one patch, or 48 cells, are one launch either way)
            assert op.launches_per_apply() > 2 if coloured else op.launches_per_apply() <= 2
        assert op.is_affine() == (mesh == "shear")
        assert op.tensor_recomputed() == (P in AUTO_DEGREES)  # the automatic default
        if reaction:
            op.set_reaction(sigma)
        op.set_tensor_recompute(False)
        assert not op.tensor_recomputed()
        streamed = _apply(pm, op, layout, u)
        err = _relerr(streamed, ref)
        print(f"apply {mesh} P={P} coloured={coloured}: streamed vs oracle {err:.3e}")
        assert err < TOL
        if P not in FORM_DEGREES:
            with pytest.raises(_lib.PmgError, match="cannot recompute its tensor"):
                op.set_tensor_recompute(True)
            assert not op.tensor_recomputed()
            continue
        op.set_tensor_recompute(True)
        assert op.tensor_recomputed()
        for rep in range(2):  # the second call: no dependence on what the first left behind
            got = _apply(pm, op, layout, u, fill=3.0 + rep)
            err, diff = _relerr(got, ref), _relerr(got, streamed)
            OBSERVED["forms"] = max(OBSERVED["forms"], diff)
            print(f"apply {mesh} P={P} coloured={coloured} call {rep}: recomputed vs oracle {err:.3e}, vs stream "
                  f"{diff:.3e} (largest so far {OBSERVED['forms']:.3e})")
            assert err < TOL and diff < TOL
        if markers:  # Dirichlet rows: y = x exactly, in both forms
            rows = np.nonzero(bc)[0]
            assert np.array_equal(got[rows], u[rows])
        op.set_tensor_recompute(None)
        assert op.tensor_recomputed() == (P in AUTO_DEGREES)


@pytest.mark.parametrize("coloured", [True, False])
def test_fused_restriction_recomputed(pm, coloured):
    from oracle import pmg_oracle as po

    part = _part(pm, "jitter")
    pc, pf = 1, 2
    lc = part.level(pc)
    Lc = pm.make_layout(lc)
    lf, Lf, fop = _operator(pm, part, pf, part.level(pf).bc_marker, coloured)
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    A = po.Laplacian(pf, _kappa(part.ncells), lf.dofmap, part.xgeom, part.geom_dofmap, lf.bc_marker)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    rng = np.random.default_rng(21)
    zu, ru = rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)
    ref = oi.reverse_interpolate(ru - A.apply(zu))
    z, r, coarse = _vec(pm, Lf, zu), _vec(pm, Lf, ru), pm.Vector(Lc)
    out = {}
    for mode in (False, True):
        fop.set_tensor_recompute(mode)
        assert fop.tensor_recomputed() == mode
        for rep in range(2):
            coarse.set(3.0)
            ip.restrict_residual(fop, z, r, coarse)
            out[mode] = coarse.data_copy()
            err = _relerr(out[mode], ref)
            print(f"fused (1,2) recomputed={mode} coloured={coloured} call {rep}: vs oracle {err:.3e}")
            assert err < TOL
    # the library's own unfused sequence in the recomputed form: q = A z, then the restriction of r - q
    q, d, c2 = pm.Vector(Lf), pm.Vector(Lf), pm.Vector(Lc)
    fop(z, q)
    d.data.copy_(r.data - q.data)
    ip.reverse_interpolate(d, c2)
    e_unfused, e_forms = _relerr(out[True], c2.data_copy()), _relerr(out[True], out[False])
    print(f"fused (1,2) coloured={coloured}: recomputed vs unfused sequence {e_unfused:.3e}, vs streamed {e_forms:.3e}")
    assert e_unfused < TOL and e_forms < TOL


CYCLE_N = (8, 8, 16)


@pytest.fixture(scope="module")
def oracle_cycles():
    """Three V-cycles from zero on the numpy oracle, computed once per hierarchy and shared."""
    cache = {}

    def get(orders, eig_ranges):
        from oracle import pmg_oracle as po

        if orders not in cache:
            mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(CYCLE_N, orders, cheb_its=3, warp=jitter(CYCLE_N))
            for s, e in zip(sm, eig_ranges):  # the device's smoother bounds: only the cycle's arithmetic is compared
                s.eig_range = e
            xo, its = np.zeros_like(b), []
            for _ in range(3):
                xo = mg.apply(b, xo)
                its.append(xo.copy())
            cache[orders] = its
        return cache[orders]

    return get


def _cycles(h, k=3):
    x = h.new_vector()
    x.set(0.0)
    out = []
    for _ in range(k):
        h.mg.apply(h.rhs[-1], x)
        out.append(x.data_copy())
    return out


def _switch(h, on):
    for op in h.operators:
        if op.degree in FORM_DEGREES:
            op.set_tensor_recompute(on)
    return [op.tensor_recomputed() for op in h.operators]


@pytest.mark.parametrize("orders", [(1, 2), (1, 2, 4)])
def test_cycles_recomputed(pm, oracle_cycles, orders):
    h = pm.PoissonHierarchy(CYCLE_N, orders, kappa=2.0, cheb_its=3, warp=jitter(CYCLE_N))
    ref = oracle_cycles(orders, h.eig_ranges)
    want_on = [p in FORM_DEGREES for p in orders]
    assert [op.tensor_recomputed() for op in h.operators] == [p in AUTO_DEGREES for p in orders]
    h.mg.set_graph(False)
    res, counts, fused = {}, {}, {}
    for on in (True, False):
        assert _switch(h, on) == (want_on if on else [False] * len(orders))
        res[on] = _cycles(h)
        counts[on], fused[on] = h.mg.apply_counts(), h.mg.fused_restrictions()
        for c, (got, want) in enumerate(zip(res[on], ref)):
            err = _relerr(got, want)
            print(f"cycle {orders} recomputed={on}, cycle {c}: rel.err vs oracle {err:.3e}")
            assert err < TOL_CYCLE
    assert counts[True] == counts[False] and fused[True] == fused[False] == len(orders) - 1
    # replayed as a graph, the switch flipped between replays: the choice is part of the graph's key
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    for i, on in enumerate((True, False, True)):
        _switch(h, on)
        got = _cycles(h)
        assert h.mg.graph_replays() == n0 + 3 * (i + 1)
        assert h.mg.apply_counts() == counts[True] and h.mg.fused_restrictions() == fused[True]
        for a, b in zip(got, res[on]):
            assert _relerr(a, b) < TOL
    h.mg.set_graph(False)


def _streams(pm, op, layout, n, seed=1):
    """An operator that must keep the stream: the report says so, forcing the form is refused with a reason, and the
    automatic choice applies exactly what `always stream` applies."""
    from pmg_dolfinx_amd import _lib

    assert not op.tensor_recomputed()
    with pytest.raises(_lib.PmgError, match="cannot recompute its tensor: "):
        op.set_tensor_recompute(True)
    assert not op.tensor_recomputed()
    u = np.random.default_rng(seed).standard_normal(n)
    auto = _apply(pm, op, layout, u)
    op.set_tensor_recompute(False)
    assert _relerr(_apply(pm, op, layout, u), auto) < NOISE
    op.set_tensor_recompute(None)
    return u, auto


@pytest.mark.parametrize("P", [3, 4])
def test_fall_back_degrees_without_the_form(pm, P):
    part = _part(pm, "jitter")
    lv, layout, op = _operator(pm, part, P, part.level(P).bc_marker)
    _streams(pm, op, layout, lv.ndofs)


def test_fall_back_curved_operator(pm):
    from test_gpu_fused_restriction import warp

    part = pm.BoxPartition((3, 3, 4), warp=warp, geom_degree=2)
    lv, layout, op = _operator(pm, part, 2, part.level(2).bc_marker, geometry_degree=2)
    _streams(pm, op, layout, lv.ndofs)


def test_fall_back_caller_tables(pm):
    from oracle import pmg_oracle as po

    part = _part(pm, "jitter")
    dphi, w3 = po.geometry_tables(2)
    lv, layout, op = _operator(pm, part, 2, part.level(2).bc_marker, dphi_geometry=dphi, G_weights=w3)
    u, got = _streams(pm, op, layout, lv.ndofs)
    own = _operator(pm, part, 2, lv.bc_marker)[2]
    assert own.tensor_recomputed()
    assert _relerr(_apply(pm, own, layout, u), got) < TOL


def test_fall_back_field_tensor_batching_and_affine_mode(pm):
    """What is set and removed on a living operator: each puts it back on the stream, and taking it away returns it to
    the recomputed form with the result it had."""
    from pmg_dolfinx_amd import _lib

    part = _part(pm, "shear")
    lv, layout, op = _operator(pm, part, 2, part.level(2).bc_marker)
    assert op.tensor_recomputed()
    u = np.random.default_rng(2).standard_normal(lv.ndofs)
    before = _apply(pm, op, layout, u)
    kq = _vec(pm, layout, np.random.default_rng(4).uniform(0.5, 1.5, lv.ndofs))
    kt = np.tile(np.array([1.5, 0.2, 0.1, 1.1, 0.3, 0.9]), (part.ncells, 1))
    changes = [
        ("field", lambda: op.set_coefficient_field(kq), lambda: op.set_coefficient_field(None)),
        ("tensor", lambda: op.set_coefficient_tensor(kt), lambda: op.set_coefficient_tensor(None)),
        ("batching", lambda: _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 64),
         lambda: _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)),
        ("affine mode", lambda: op.set_geometry_mode("affine"), lambda: op.set_geometry_mode("stored")),
    ]
    for name, put, take in changes:
        put()
        try:
            u2, with_it = _streams(pm, op, layout, lv.ndofs, seed=2)
            if name in ("batching", "affine mode"):  # the same operator through another data path
                assert _relerr(with_it, before) < TOL
            else:
                assert _relerr(with_it, before) > 1e-2
        finally:
            take()
        assert op.tensor_recomputed(), name
        assert _relerr(_apply(pm, op, layout, u), before) < NOISE, name


def test_fall_back_fp32_cycle(pm):
    """The FP32 cycle applies the float tensor and never reads the switch: its result does not move with it.  (The
    report speaks of the operator's FP64 application.)  Bound: the same float kernels on the same bits twice, whose
    atomics arrive in any order -- a few float roundings (6e-8) carried through one cycle."""
    n = (4, 4, 16)
    h = pm.PoissonHierarchy(n, (1, 2), kappa=2.0, cheb_its=3, warp=jitter(n))
    h.mg.set_precision("fp32")
    res = {}
    for on in (True, False):
        _switch(h, on)
        res[on] = _cycles(h, 1)[0]
    err = _relerr(res[True], res[False])
    print(f"fp32 cycle, switch on against off: {err:.3e}")
    assert err < 1e-5
    h.mg.set_precision("fp64")


def test_environment_switch(pm, monkeypatch):
    part = _part(pm, "jitter")
    bc = part.level(2).bc_marker
    monkeypatch.setenv("PMG_TENSOR_RECOMPUTE", "0")
    assert not _operator(pm, part, 2, bc)[2].tensor_recomputed()
    monkeypatch.setenv("PMG_TENSOR_RECOMPUTE", "1")
    assert _operator(pm, part, 2, bc)[2].tensor_recomputed()
    assert not _operator(pm, part, 4, part.level(4).bc_marker)[2].tensor_recomputed()  # (no error: it streams)
