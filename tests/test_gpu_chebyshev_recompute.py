"""The recomputed form of the Chebyshev smooth (ChebRecomputeF in csrc/vector.hip, cheb_iterate in csrc/solvers.hip,
pmg_chebyshev_set_recompute) against the stored form, the oracle, and the configurations that must keep the stored loop.

Mesh: 4 x 4 x 16 cells at degree 4, the smallest box with all eight patch colours (2 x 2 x 2 patches); 17 x 17 x 65 =
18 785 dofs, odd, so the scalar tail of every vector kernel runs.  Hierarchy (1, 2, 4) with set_merge_threshold(0):
no level merges its colours into an accumulating launch, so every level qualifies and the zero-guess variants run on
the coarse levels.

Bit for bit.  The two forms share the helpers that fix the roundings of the correction formula (cheb_correction,
cheb_first_correction) and form the residual in the same order, so given the same operator products they agree bit
for bit.  The operator's products themselves are not reproducible on that mesh: a dof shared by more than two cells is
summed in the order the atomics arrive, and two runs of the STORED form differ there in a few hundred entries (observed
on an MI355X: 1.2e-15 after a solve, 2.8e-16 after a cycle; the recomputed form against the stored one: the same
figures).  So equality is asserted where it is defined -- on a column of 1 x 1 x 16 cells, where every dof has at most
two addends (a + b = b + a) and the stored form repeats itself bit for bit, which the tests check first: solves, cycles,
replayed cycles and every alignment of the caller's vectors -- and on the 4 x 4 x 16 mesh mode 1 against mode 0 is held
to TOL_SOLVE.  Against the oracle the bars are TOL_SOLVE and TOL_RNORM of tests/test_gpu_fp64_vector_kernels.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_fp64_vector_kernels import TOL_RNORM, TOL_SOLVE, _on, _relerr, _same, _Span  # noqa: E402

N = (4, 4, 16)
COLUMN = (1, 1, 16)  # 5 x 5 x 65 = 1625 dofs at degree 4, odd; every dof belongs to one or two cells
ORDERS = (1, 2, 4)
TOL_FP32 = 1e-4  # one FP32 cycle against the FP64 oracle (tests/test_gpu_mixed_precision.py)
OFFSETS = ((0, 0), (1, 1), (1, 0), (0, 1))  # (rhs, iterate): doubles past a 16-byte boundary


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _hierarchy(pm, n=N, coloured=True, **kw):
    try:
        pm.set_merge_threshold(0 if coloured else -1)
        h = pm.PoissonHierarchy(n, ORDERS, kappa=2.0, cheb_its=3, **kw)
    finally:
        pm.set_merge_threshold(-1)
    h.mg.set_graph(False)
    return h


@pytest.fixture(scope="module")
def h(pm):
    h = _hierarchy(pm, warp=warp)
    assert h.levels[-1].size_local == 18785
    # the degree-4 level launches its eight colours one by one; the coarser levels are one patch each, a single plain
    # launch: no level accumulates into a zeroed output, so every level qualifies
    assert [op.launches_per_apply() for op in h.operators][-1] >= 8
    return h


@pytest.fixture(scope="module")
def column(pm):
    """The column of cells; Dirichlet dofs on the face x = 0 only (the degree-1 level keeps free dofs)."""
    hc = _hierarchy(pm, n=COLUMN, dirichlet=lambda c: c[:, 0] < 1e-12)
    assert [lv.size_local for lv in hc.levels] == [2 * 2 * 17, 3 * 3 * 33, 5 * 5 * 65]
    return hc


@pytest.fixture(scope="module")
def oracle(h):
    """The numpy oracle with the device's smoother bounds; three cycles from zero per k, computed once and shared."""
    from oracle import pmg_oracle as po

    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(N, ORDERS, cheb_its=3, warp=warp)
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    cache = {}

    def cycles(k):
        if k not in cache:
            for s in sm:
                s.set_max_iterations(k)
            xo, its, rns = np.zeros_like(b), [], []
            for _ in range(3):
                xo = mg.apply(b, xo, compute_rnorm=True)
                its.append(xo.copy())
                rns.append(mg.rnorm)
            cache[k] = (its, rns)
        return cache[k]

    return dict(ops=ops, b=b, cycles=cycles, po=po)


def _set(h, k=None, mode=None):
    for sm in h.smoothers:
        if k is not None:
            sm.set_max_iterations(k)
        sm.set_recompute(mode)


def _counts(h):
    return [sm.recomputed() for sm in h.smoothers]


def _cycles(pm, h, off_b=0, off_x=0, n=3):
    """n cycles from x = 0 on vectors at the given offsets from a 16-byte boundary: iterates and residual norms."""
    lay, nd = h.layouts[-1], h.levels[-1].size_local
    sb, sx = _Span(nd, off_b).put(h.rhs[-1].data_copy()), _Span(nd, off_x, fill=0.0)
    vb, vx = _on(pm, lay, sb), _on(pm, lay, sx)
    its, rns = [], []
    for _ in range(n):
        rns.append(h.mg.apply(vb, vx, verbose=True))
        its.append(sx.get())
    sb.assert_guards()
    sx.assert_guards()
    return its, rns


def _check_oracle(what, got, rns, ref):
    for c, (g, rn, xo, rno) in enumerate(zip(got, rns, *ref)):
        e, en = _relerr(g, xo), abs(rn - rno) / max(rno, 1e-30)
        print(f"{what}, cycle {c}: iterate vs oracle {e:.3e} (bar {TOL_SOLVE:.0e}), rnorm {en:.3e} (bar {TOL_RNORM:.0e})")
        assert e < TOL_SOLVE and en < TOL_RNORM


def _check_forms(what, new, stored):
    for c, (a, b) in enumerate(zip(new, stored)):
        e = _relerr(a, b)
        print(f"{what}, cycle {c}: recomputed vs stored {e:.3e} (bar {TOL_SOLVE:.0e})")
        assert e < TOL_SOLVE


def _solves(pm, h, level, k, x0, b):
    """Chebyshev.solve in mode 0, 0 again and 1 at every alignment: results by (run, off_b, off_x)."""
    sm, op, lay = h.smoothers[level], h.operators[level], h.layouts[level]
    nd = h.levels[level].size_local
    assert nd % 2 == 1
    sm.set_max_iterations(k)
    got = {}
    for run, mode in (("stored", 0), ("again", 0), ("recomputed", 1)):
        sm.set_recompute(mode)
        before = sm.recomputed()
        for off_b, off_x in OFFSETS:
            sb, sx = _Span(nd, off_b).put(b), _Span(nd, off_x).put(x0)
            sm.solve(op, _on(pm, lay, sx), _on(pm, lay, sb))
            got[run, off_b, off_x] = sx.get()
            sb.assert_guards()
            sx.assert_guards()
        assert sm.recomputed() == before + (len(OFFSETS) if mode else 0)  # which path ran
    sm.set_recompute(None)
    return got


def _start(kind, nd, seed):
    return np.random.default_rng(seed).standard_normal(nd) if kind == "random" else np.zeros(nd)


@pytest.mark.parametrize("level", [2, 1])
@pytest.mark.parametrize("start", ["random", "zero"])
@pytest.mark.parametrize("k", [2, 3])
def test_solve_equals_the_stored_form_bit_for_bit(pm, column, k, start, level):
    nd = column.levels[level].size_local
    x0 = _start(start, nd, 10 * k + level)
    got = _solves(pm, column, level, k, x0, column.rhs[level].data_copy())
    ref = got["stored", 0, 0]
    assert np.abs(ref - x0).max() > 0 and ref[-1] != x0[-1]  # the smooth did something, on the tail element too
    for off in OFFSETS:
        assert _same(got[("again",) + off], ref), off  # what the assertion below rests on: the stored form repeats
    for off in OFFSETS:
        assert _same(got[("recomputed",) + off], ref), off  # both bodies (pair, scalar) of the three kernels


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("k", [2, 3])
def test_cycles_equal_the_stored_form_bit_for_bit(pm, column, k, fused):
    """Eager and replayed, aligned and not: pre-smooths that feed the fused restriction (r and z written), post-smooths,
    and the zero-guess variants on the coarser levels."""
    column.mg.set_fused_restriction(None if fused else 0)
    try:
        _set(column, k, 0)
        stored, rn_stored = _cycles(pm, column)
        again, _ = _cycles(pm, column)
        assert all(_same(a, b) for a, b in zip(again, stored))  # the stored form repeats on this mesh
        assert column.mg.fused_restrictions() == (len(ORDERS) - 1 if fused else 0)
        _set(column, k, 1)
        c0 = _counts(column)
        for off in OFFSETS:
            new, rn_new = _cycles(pm, column, *off)
            assert all(_same(a, b) for a, b in zip(new, stored)), off
            assert rn_new == rn_stored
        per_cycle = (1, 2, 2) if fused else (1, 1, 1)
        assert _counts(column) == [a + 3 * len(OFFSETS) * d for a, d in zip(c0, per_cycle)]
        column.mg.set_graph(True)
        n0 = column.mg.graph_replays()
        replayed, _ = _cycles(pm, column)
        assert column.mg.graph_replays() >= n0 + 3
        assert all(_same(a, b) for a, b in zip(replayed, stored))
    finally:
        column.mg.set_graph(False)
        column.mg.set_fused_restriction(None)
        _set(column, 3, None)


@pytest.mark.parametrize("level", [2, 1])
@pytest.mark.parametrize("start", ["random", "zero"])
@pytest.mark.parametrize("k", [2, 3])
def test_solve_against_the_oracle_and_the_stored_form(pm, h, oracle, k, start, level):
    po = oracle["po"]
    nd = h.levels[level].size_local
    b = h.rhs[level].data_copy()
    x0 = _start(start, nd, 10 * k + level)
    ref = po.Chebyshev(h.eig_ranges[level], k).solve(oracle["ops"][level], x0.copy(), b)
    got = _solves(pm, h, level, k, x0, b)
    for off in OFFSETS:
        e, d = _relerr(got[("recomputed",) + off], ref), _relerr(got[("recomputed",) + off], got[("stored",) + off])
        again = _relerr(got[("again",) + off], got[("stored",) + off])
        print(f"solve k = {k}, {start} guess, level {level}, offsets {off}: recomputed vs oracle {e:.3e}, vs stored "
              f"{d:.3e} (bars {TOL_SOLVE:.0e}); stored vs stored again {again:.3e}")
        assert e < TOL_SOLVE and d < TOL_SOLVE


@pytest.mark.parametrize("k", [2, 3])
def test_three_cycles_with_the_fused_restriction(pm, h, oracle, k):
    _set(h, k, 0)
    c0 = _counts(h)
    stored, rn_stored = _cycles(pm, h)
    assert _counts(h) == c0
    applies, fused = h.mg.apply_counts(), h.mg.fused_restrictions()
    assert fused == len(ORDERS) - 1
    _set(h, k, 1)
    new, rn_new = _cycles(pm, h)
    print(f"k = {k}: recomputed smooths per level {c0} -> {_counts(h)}, applies {applies}, fused {fused}")
    # per cycle: a pre- and a post-smooth on the two upper levels, the coarse level's one smooth from zero
    assert _counts(h) == [a + 3 * d for a, d in zip(c0, (1, 2, 2))]
    assert h.mg.apply_counts() == applies and h.mg.fused_restrictions() == fused
    _check_forms(f"k = {k}", new, stored)
    _check_oracle(f"k = {k}, recomputed", new, rn_new, oracle["cycles"](k))
    _set(h, 3, None)


def test_graph_replay_and_switching_between_replays(pm, h, oracle):
    _set(h, 3, 1)
    eager, _ = _cycles(pm, h)
    lay, nd = h.layouts[-1], h.levels[-1].size_local
    sb, sx = _Span(nd, 0).put(h.rhs[-1].data_copy()), _Span(nd, 0, fill=0.0)
    vb, vx = _on(pm, lay, sb), _on(pm, lay, sx)
    h.mg.set_graph(True)
    try:
        for first in (True, False):  # captured, then replayed from the cache
            for mode, step in ((1, (1, 2, 2)), (0, (0, 0, 0)), (1, (1, 2, 2))):
                _set(h, None, mode)
                sx.view.fill_(0.0)
                its = []
                for _ in range(3):
                    c, n0 = _counts(h), h.mg.graph_replays()
                    h.mg.apply(vb, vx)
                    assert h.mg.graph_replays() == n0 + 1
                    assert _counts(h) == [a + d for a, d in zip(c, step)], (first, mode)  # no stale graph
                    its.append(sx.get())
                _check_forms(f"replayed, mode {mode}, {'captured' if first else 'cached'} against eager", its, eager)
    finally:
        h.mg.set_graph(False)
        _set(h, 3, None)


def test_misaligned_caller_vectors(pm, h, oracle):
    """Right-hand side and iterate 8 bytes past a 16-byte boundary: the kernels that touch them run their scalar body
    over the whole level."""
    _set(h, 3, 1)
    aligned, rn = _cycles(pm, h)
    for off_b, off_x in OFFSETS[1:]:
        got, rn_got = _cycles(pm, h, off_b, off_x)
        _check_oracle(f"offsets {off_b}, {off_x}", got, rn_got, oracle["cycles"](3))
        _check_forms(f"offsets {off_b}, {off_x} against aligned", got, aligned)
    _set(h, 3, None)


@pytest.mark.parametrize("k", [1, 4, 5])
def test_fall_back_other_step_counts(pm, h, oracle, k):
    _set(h, k, 1)
    c0 = _counts(h)
    got, rn = _cycles(pm, h)
    assert _counts(h) == c0
    _check_oracle(f"k = {k}", got, rn, oracle["cycles"](k))
    _set(h, 3, None)


def test_fall_back_unfused_restriction(pm, h, oracle):
    """Without the fusion the pre-smooth returns its residual in the split form and keeps the stored loop; the
    post-smooth and the coarse level's smooth still qualify."""
    _set(h, 3, 1)
    h.mg.set_fused_restriction(0)
    try:
        c0 = _counts(h)
        got, rn = _cycles(pm, h)
        assert h.mg.fused_restrictions() == 0
        assert _counts(h) == [a + 3 for a in c0]
        _check_oracle("unfused", got, rn, oracle["cycles"](3))
    finally:
        h.mg.set_fused_restriction(None)
        _set(h, 3, None)


def test_fall_back_fp32_cycle(pm, h, oracle):
    _set(h, 3, 1)
    h.mg.set_precision("fp32")
    try:
        c0 = _counts(h)
        x = h.new_vector()
        x.set(0.0)
        h.mg.apply(h.rhs[-1], x)
        assert _counts(h) == c0
        e = _relerr(x.data_copy(), oracle["cycles"](3)[0][0])
        print(f"FP32 cycle vs oracle {e:.3e} (bar {TOL_FP32:.0e})")
        assert e < TOL_FP32
    finally:
        h.mg.set_precision("fp64")
        _set(h, 3, None)


def test_fall_back_merged_levels(pm, oracle):
    """The default merge threshold: the degree-4 level of this mesh runs its colours as one accumulating launch, whose
    output the smoother's kernels clear behind themselves -- the stored loop, whatever the mode.  (The coarser levels
    are one patch each: nothing to merge, they qualify as before.)"""
    hm = _hierarchy(pm, coloured=False, warp=warp)
    assert hm.operators[-1].launches_per_apply() <= 2
    _set(hm, 3, 1)
    got, rn = _cycles(pm, hm)
    print(f"merged: recomputed smooths per level {_counts(hm)}")
    assert _counts(hm) == [3, 6, 0]
    _check_oracle("merged", got, rn, oracle["cycles"](3))


def test_fall_back_assembled_level(pm, oracle):
    """An assembled matrix on the finest level: its smooths are the matrix's and keep the stored loop."""
    ha = _hierarchy(pm, warp=warp, assembled_levels=(2,))
    _set(ha, 3, 1)
    got, rn = _cycles(pm, ha)
    assert _counts(ha) == [3, 6, 0]
    _check_oracle("assembled finest level", got, rn, oracle["cycles"](3))


def test_automatic_mode_follows_the_streaming_threshold(pm, h):
    """Automatic: on where the vectors are streamed (4 Mi dofs and more, checked at full size by the config-2 tests),
    off on levels as small as these."""
    _set(h, 3, None)
    c0 = _counts(h)
    _cycles(pm, h, n=1)
    assert _counts(h) == c0
