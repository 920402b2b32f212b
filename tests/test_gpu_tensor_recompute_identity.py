"""The recomputed tensor of the degree-4 apply (pmg_laplacian_set_tensor_recompute_identity): the column kernel and the
fused (4, 2) restrict kernel take TensorStream's GEO_RECOMPUTE form with their transposes by the barycentric identity
(transposes_by_identity, pmg-dolfinx_amd/csrc/stiffness_column.hpp).  Form on and off against the oracle and against
each other; V-cycles, eager and replayed; every configuration in which a degree-4 operator must keep streaming G; and
the independence of this switch from pmg_laplacian_set_tensor_recompute.

Meshes, helpers and bounds are those of tests/test_gpu_tensor_recompute.py: 1e-12 of max |y| for one application or
transfer, 1e-10 after V-cycles, NOISE = 1e-14 for the same kernels on the same bits twice.  The two forms differ by
rounding of G, by where kappa multiplies (the cell's input instead of its fluxes) and by the identity's sums: same
value to rounding; the largest difference seen is printed and held to the 1e-12 bar."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_tensor_recompute import (CYCLE_N, NOISE, TOL, TOL_CYCLE, _apply, _cycles, _kappa, _operator, _part,
                                       _reference, _relerr, _vec, jitter, oracle_cycles, pm)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P4 = 4
OBSERVED = {"forms": 0.0}


def _auto(op):
    """The automatic choice of this library at degree 4 (recompute_identity_default, laplacian.hip), read from a fresh
    operator: the tests hold in either case."""
    op.set_tensor_recompute_identity(None)
    return op.tensor_recomputed_identity()


@pytest.mark.parametrize("reaction", [False, True])
@pytest.mark.parametrize("markers", [True, False])
@pytest.mark.parametrize("mesh", ["jitter", "shear", "frames"])
def test_apply_identity_form_against_stream_and_oracle(pm, mesh, markers, reaction):
    part = _part(pm, mesh)
    bc, sigma, u, ref = _reference(part, mesh, P4, markers, reaction)
    for coloured in (True, False):
        lv, layout, op = _operator(pm, part, P4, bc, coloured)
        if mesh == "jitter":  # (one patch, or 48 cells, are one launch either way)
            assert op.launches_per_apply() > 2 if coloured else op.launches_per_apply() <= 2
        assert op.is_affine() == (mesh == "shear")
        if reaction:
            op.set_reaction(sigma)
        op.set_tensor_recompute_identity(False)
        assert not op.tensor_recomputed_identity()
        streamed = _apply(pm, op, layout, u)
        err = _relerr(streamed, ref)
        print(f"apply {mesh} P=4 coloured={coloured}: streamed vs oracle {err:.3e}")
        assert err < TOL
        op.set_tensor_recompute_identity(True)
        assert op.tensor_recomputed_identity()
        for rep in range(2):  # the second call: another fill of y, no dependence on what the first left behind
            got = _apply(pm, op, layout, u, fill=3.0 + rep)
            err, diff = _relerr(got, ref), _relerr(got, streamed)
            OBSERVED["forms"] = max(OBSERVED["forms"], diff)
            print(f"apply {mesh} P=4 coloured={coloured} call {rep}: recomputed vs oracle {err:.3e}, vs stream "
                  f"{diff:.3e} (largest so far {OBSERVED['forms']:.3e})")
            assert err < TOL and diff < TOL
            if markers:  # Dirichlet rows: y = x exactly
                rows = np.nonzero(bc)[0]
                assert np.array_equal(got[rows], u[rows])
        op.set_tensor_recompute_identity(None)


@pytest.mark.parametrize("coloured", [True, False])
def test_fused_restriction_identity_form(pm, coloured):
    from oracle import pmg_oracle as po

    part = _part(pm, "jitter")
    pc, pf = 2, 4
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
        fop.set_tensor_recompute_identity(mode)
        assert fop.tensor_recomputed_identity() == mode
        for rep in range(2):
            coarse.set(3.0)
            ip.restrict_residual(fop, z, r, coarse)
            out[mode] = coarse.data_copy()
            err = _relerr(out[mode], ref)
            print(f"fused (2,4) recomputed={mode} coloured={coloured} call {rep}: vs oracle {err:.3e}")
            assert err < TOL
    e_forms = _relerr(out[True], out[False])
    print(f"fused (2,4) coloured={coloured}: recomputed vs streamed {e_forms:.3e}")
    assert e_forms < TOL


def _switch(h, on):
    for op in h.operators:
        if op.degree == P4:
            op.set_tensor_recompute_identity(on)
    return [op.tensor_recomputed_identity() for op in h.operators]


def test_cycles_identity_form(pm, oracle_cycles):
    orders = (1, 2, 4)
    h = pm.PoissonHierarchy(CYCLE_N, orders, kappa=2.0, cheb_its=3, warp=jitter(CYCLE_N))
    ref = oracle_cycles(orders, h.eig_ranges)
    old = [op.tensor_recomputed() for op in h.operators]
    h.mg.set_graph(False)
    res, counts, fused = {}, {}, {}
    for on in (True, False):
        assert _switch(h, on) == [False, False, on]
        assert [op.tensor_recomputed() for op in h.operators] == old  # the other switch has not moved
        res[on] = _cycles(h)
        counts[on], fused[on] = h.mg.apply_counts(), h.mg.fused_restrictions()
        for c, (got, want) in enumerate(zip(res[on], ref)):
            err = _relerr(got, want)
            print(f"cycle {orders} identity form={on}, cycle {c}: rel.err vs oracle {err:.3e}")
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
    automatic choice applies exactly what `never` applies."""
    from pmg_dolfinx_amd import _lib

    assert not op.tensor_recomputed_identity()
    with pytest.raises(_lib.PmgError, match="cannot recompute its tensor: ."):
        op.set_tensor_recompute_identity(True)
    assert not op.tensor_recomputed_identity()
    u = np.random.default_rng(seed).standard_normal(n)
    before = _apply(pm, op, layout, u)
    op.set_tensor_recompute_identity(False)
    assert not op.tensor_recomputed_identity()
    assert _relerr(_apply(pm, op, layout, u), before) < NOISE
    return u, before


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_fall_back_other_degrees(pm, P):
    part = _part(pm, "jitter")
    lv, layout, op = _operator(pm, part, P, part.level(P).bc_marker)
    old = op.tensor_recomputed()
    _streams(pm, op, layout, lv.ndofs)
    op.set_tensor_recompute_identity(None)
    assert op.tensor_recomputed() == old  # (degrees 1 and 2: their own form is untouched)


def test_fall_back_curved_operator(pm):
    from test_gpu_fused_restriction import warp

    part = pm.BoxPartition((3, 3, 4), warp=warp, geom_degree=2)
    lv, layout, op = _operator(pm, part, P4, part.level(P4).bc_marker, geometry_degree=2)
    _streams(pm, op, layout, lv.ndofs)


def test_fall_back_caller_tables(pm):
    from oracle import pmg_oracle as po

    part = _part(pm, "jitter")
    dphi, w3 = po.geometry_tables(P4)
    lv, layout, op = _operator(pm, part, P4, part.level(P4).bc_marker, dphi_geometry=dphi, G_weights=w3)
    u, got = _streams(pm, op, layout, lv.ndofs)
    own = _operator(pm, part, P4, lv.bc_marker)[2]
    own.set_tensor_recompute_identity(True)
    assert own.tensor_recomputed_identity()
    assert _relerr(_apply(pm, own, layout, u), got) < TOL


def test_fall_back_field_tensor_batching_and_affine_mode(pm):
    """What is set and removed on a living degree-4 operator: each puts it back on the stream, and taking it away
    returns it to the recomputed form with the result it had."""
    from pmg_dolfinx_amd import _lib

    part = _part(pm, "shear")
    lv, layout, op = _operator(pm, part, P4, part.level(P4).bc_marker)
    op.set_tensor_recompute_identity(True)
    assert op.tensor_recomputed_identity()
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
            assert not op.tensor_recomputed_identity(), name
            with_it = _apply(pm, op, layout, u)
            if name in ("batching", "affine mode"):  # the same operator through another data path
                assert _relerr(with_it, before) < TOL
            else:
                assert _relerr(with_it, before) > 1e-2
        finally:
            take()
        assert op.tensor_recomputed_identity(), name  # by itself: the request stands, eligibility is re-evaluated
        assert _relerr(_apply(pm, op, layout, u), before) < NOISE, name
        put()
        try:
            _, again = _streams(pm, op, layout, lv.ndofs, seed=2)  # (seed 2: the same vector as u)
            assert _relerr(again, with_it) < NOISE, name
        finally:
            take()
        op.set_tensor_recompute_identity(True)  # (`never` was the last setting of _streams)
        assert op.tensor_recomputed_identity(), name
        assert _relerr(_apply(pm, op, layout, u), before) < NOISE, name


def test_fall_back_chain_form(pm, monkeypatch):
    """(4, 4, 64): sixteen 2 x 2 x 8 patches in a row, the smallest mesh on which chains exist
    (tests/test_gpu_reaction.py::test_chain_form_requested).  In chain form the operator streams; out of it the form
    is available again."""
    monkeypatch.setenv("PMG_CHAIN", "2")
    part = pm.BoxPartition((4, 4, 64))
    lv, layout, op = _operator(pm, part, P4, part.level(P4).bc_marker, coloured=True)
    assert op.chain_available() and op.chain_form()
    u, chained = _streams(pm, op, layout, lv.ndofs)
    op.set_chain_form(False)
    op.set_tensor_recompute_identity(True)
    assert op.tensor_recomputed_identity()
    assert _relerr(_apply(pm, op, layout, u), chained) < TOL
    op.set_chain_form(True)
    assert not op.tensor_recomputed_identity()
    assert _relerr(_apply(pm, op, layout, u), chained) < NOISE


def test_fall_back_fp32_cycle(pm):
    """The FP32 cycle applies the float tensor and never reads the switch: its result does not move with it.  Bound: as
    tests/test_gpu_tensor_recompute.py::test_fall_back_fp32_cycle."""
    n = (4, 4, 16)
    h = pm.PoissonHierarchy(n, (1, 2, 4), kappa=2.0, cheb_its=3, warp=jitter(n))
    h.mg.set_precision("fp32")
    res = {}
    for on in (True, False):
        _switch(h, on)
        res[on] = _cycles(h, 1)[0]
    err = _relerr(res[True], res[False])
    print(f"fp32 cycle, identity switch on against off: {err:.3e}")
    assert err < 1e-5
    h.mg.set_precision("fp64")


def test_independent_of_the_low_degree_switch(pm):
    from pmg_dolfinx_amd import _lib

    part = _part(pm, "jitter")
    lv, layout, op = _operator(pm, part, P4, part.level(P4).bc_marker)
    auto = _auto(op)
    for mode in (True, False, None):
        op.set_tensor_recompute_identity(mode)
        want = auto if mode is None else mode
        assert op.tensor_recomputed_identity() == want and not op.tensor_recomputed()
        with pytest.raises(_lib.PmgError, match="cannot recompute its tensor: the form exists at degrees 1 and 2 only"):
            op.set_tensor_recompute(True)
        assert op.tensor_recomputed_identity() == want and not op.tensor_recomputed()
        for old in (False, None):  # the old switch does not move the new report
            op.set_tensor_recompute(old)
            assert op.tensor_recomputed_identity() == want and not op.tensor_recomputed()
    lv2, layout2, op2 = _operator(pm, part, 2, part.level(2).bc_marker)
    for old in (True, False):
        op2.set_tensor_recompute(old)
        assert op2.tensor_recomputed() == old and not op2.tensor_recomputed_identity()
        op2.set_tensor_recompute_identity(False)
        assert op2.tensor_recomputed() == old


def test_environment_switch(pm, monkeypatch):
    part = _part(pm, "jitter")
    bc4, bc2 = part.level(P4).bc_marker, part.level(2).bc_marker
    monkeypatch.setenv("PMG_TENSOR_RECOMPUTE_IDENTITY", "0")
    assert not _operator(pm, part, P4, bc4)[2].tensor_recomputed_identity()
    assert _operator(pm, part, 2, bc2)[2].tensor_recomputed()  # (the other switch's default is untouched)
    monkeypatch.setenv("PMG_TENSOR_RECOMPUTE_IDENTITY", "1")
    assert _operator(pm, part, P4, bc4)[2].tensor_recomputed_identity()
    op2 = _operator(pm, part, 2, bc2)[2]  # (no error: it keeps its own form)
    assert op2.tensor_recomputed() and not op2.tensor_recomputed_identity()
    monkeypatch.delenv("PMG_TENSOR_RECOMPUTE_IDENTITY")
    monkeypatch.setenv("PMG_TENSOR_RECOMPUTE", "1")  # the old environment switch does not reach degree 4
    op = _operator(pm, part, P4, bc4)[2]
    assert not op.tensor_recomputed() and op.tensor_recomputed_identity() == _auto(op)


def test_abi_of_the_pair(built):
    """Header, binding and export agree for the two entry points (tests/test_abi.py checks all declared symbols; this
    names the pair), and both report -1 / fail for NULL without a device."""
    import ctypes
    import os

    from pmg_dolfinx_amd import _lib

    names = ("pmg_laplacian_set_tensor_recompute_identity", "pmg_laplacian_tensor_recomputed_identity")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmg_amd.h")).read()
    L = _lib.lib()
    for name in names:
        assert name in _lib.exported_symbols() and f"int {name}(pmg_laplacian op" in header and hasattr(L, name)
    assert L.pmg_laplacian_tensor_recomputed_identity(ctypes.c_void_p(0)) == -1
    assert L.pmg_laplacian_set_tensor_recompute_identity(ctypes.c_void_p(0), 1) != 0
