"""The FP64 vector, smoother and CG kernels (csrc/vector.hip and the loops of csrc/solvers.hip) branch by branch.

Every element-wise kernel has a double2 body (`pair`, taken when all operands are 16-byte aligned) and a scalar body
(`one`: the whole vector when an operand is only 8-byte aligned, else the trailing element of an odd length).  The
tests below run both: vectors are views into larger allocations, starting on a 16-byte boundary or 8 bytes past one,
with guard elements on both sides that must come back untouched.

A. set / scale / copy / axpy / pointwise_mult through the C ABI: lengths around a wavefront, a block, the grid cap of
   `ew_blocks` (2048 blocks of 256 threads: 524 288 items of the scalar kernel, 1 048 576 doubles of the pair kernel)
   and a few million; layouts with and without ghosts; every operand alignment; the in-place forms.
B. inner_product / squared_norm / norm(l2, linf) on the same grid plus the lengths around the RED_BLOCKS cap; sums
   against math.fsum of exact products (float32-valued inputs: a product of two has 48 significant bits);
   cancellation; linf exactly; bit-identical repeats; NaN through every reduction.
C. cheb_iterate: k = 0 .. 5 on one, two and three levels, cell-form (ResidualUpdated) and patch-form (ResidualSplit)
   transfers, merged (ThenClearF, clear_q) and coloured launch plans, levels of odd length whose last dof is an
   interior dof (Dirichlet on the face x = 0 only, or a permuted numbering), misaligned caller vectors, two ranks as
   threads (ghosts), and the streaming sizes (4 << 20 dofs) against the C oracle.
D. cg_iterate with the diagonal, a V-cycle and the flexible variant (on one rank over a cycle with an inner CG, so that
   the flexible term is not rounding noise), aligned and misaligned, one rank and two.

Which `one` bodies the misaligned caller vectors reach as WHOLE-level kernels: the passes that read b or touch x on the
finest level -- ChebInitF (b), ChebStepF both BOTH forms (x), ChebLastF with assign = 0 (x), AddF (x), ThenClearF
around them, AxpyF (b), CgUpdateF and CgUpdate2F (x).  The work vectors of the library are its own allocations and
stay aligned, so ChebFirstF, ChebLastF with assign = 1, ChebResidualF, MulF and CgDirectionF run `one` only for the
tail element of an odd level (MaskBcF has one body per entry anyway): for those the interior-tail hierarchies are the
cover -- a wrong `one` changes the last dof, which is free there and enters every later application.

References are numpy / math.fsum / the oracles, in FP64 or better; outputs start as NaN.  The tolerances are the
project's FP64 bars, not derived from the measurements noted next to them."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# largest error seen per group in this process (printed when the module is done; read when the notes are refreshed)
OBSERVED = {}

TOL_VEC = 1e-12  # A: axpy, per element relative to |alpha x| + |y| (observed on an MI355X: 2.2e-16)
TOL_SUM = 1e-12  # B: sums, relative to sum |a_i b_i| (observed 4.1e-17; with cancellation 9.3e-18); squared and l2
#                     norm relative to themselves (observed 2.2e-16)
TOL_SOLVE = 1e-10  # C: iterate after a smoother solve or a V-cycle, max norm (observed 1.3e-15; two ranks 7.5e-16;
#                       below / above the streaming threshold 3.7e-16 / 4.8e-16, two-level cycle above it 5.5e-16)
TOL_RNORM = 1e-9  # C: the cycle's residual norm, as test_vcycle_parity (observed 7.7e-15; two ranks 5.7e-13)
TOL_CG = 1e-9  # D: alpha, beta and the iterate of CG (observed 2.6e-13, 6.1e-12, 1.2e-15; two ranks 8.1e-14,
#                    1.1e-12, 1.2e-15)
# aligned against misaligned runs of the same case are not required to agree bit for bit (largest difference observed:
# 0 in A, 4.1e-17 of sum |a_i b_i| in B, 4.4e-16 in C, 5.3e-16 in D)

SENTINEL = -1.2345e77  # guard elements around every view
GHOST = 1e300  # ghost entries that no owned-range kernel may touch and no reduction may read
PAD = 2

# around a wavefront, a block, two blocks, the grid cap of the scalar kernel (2048 * 256 items), of the pair kernel
# (2048 * 256 pairs), and a few million
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 524287, 524288, 524289, 1048575, 1048576, 1048577,
           1048578, 1048579, 3000001]
# ... and the RED_BLOCKS = 1024 cap of the partial kernels: 1024 * 256 entries (linf), 1024 * 256 pairs (dot)
RED_LENGTHS = LENGTHS + [262143, 262144, 262145]


def _check(what, err, tol):
    err = float(err)
    OBSERVED[what] = max(OBSERVED.get(what, 0.0), err)
    print(f"{what}: {err:.3e} (bar {tol:.0e})")
    assert err < tol, (what, err, tol)


def _note(what, v):
    OBSERVED[what] = max(OBSERVED.get(what, 0.0), float(v))


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    yield pm
    print("OBSERVED", {k: f"{v:.3e}" for k, v in sorted(OBSERVED.items())})


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class _Span:
    """n doubles inside a larger allocation: on a 16-byte boundary (off = 0) or 8 bytes past one (off = 1)."""

    def __init__(self, n, off, fill=float("nan")):
        self.n, self.off = int(n), int(off)
        self.base = torch.full((self.n + 2 * PAD + 2,), SENTINEL, dtype=torch.float64, device="cuda")
        assert self.base.data_ptr() % 16 == 0
        self.lo = PAD + self.off
        self.view = self.base[self.lo: self.lo + self.n]
        assert self.view.data_ptr() % 16 == 8 * self.off
        self.view.fill_(fill)

    def put(self, a):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
        return self

    def get(self):
        return self.view.cpu().numpy()

    @property
    def p(self):
        return C.c_void_p(self.view.data_ptr())

    def assert_guards(self):
        lo, hi = self.base[: self.lo].cpu().numpy(), self.base[self.lo + self.n:].cpu().numpy()
        assert np.all(lo == SENTINEL) and np.all(hi == SENTINEL), "a guard element next to the vector was written"


def _on(pm, layout, span):
    """A Vector of `layout` whose storage is the span's view."""
    v = pm.Vector(layout)
    assert span.n == layout.total
    v._x = span.view
    return v


def _abi(pm, name, *args):
    return pm._lib.call(name, *args, pm._lib.current_stream())


def _same(a, b):
    """Equal bit for bit (NaN == NaN, +0 != -0)."""
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# A. element-wise kernels
# ---------------------------------------------------------------------------------------------------------------------


def _inputs(n, ghosts, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(n + ghosts), rng.standard_normal(n + ghosts)
    out0 = np.full(n + ghosts, np.nan)
    out0[n:] = GHOST * (1.0 + np.arange(ghosts) / 8.0)  # the ghosts of an output: distinct, and they must stay
    return a, b, out0


@pytest.mark.parametrize("ghosts", [0, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_set_and_scale_act_on_owned_and_ghost_entries(pm, n, ghosts):
    lay = pm.Layout(n, num_ghosts=ghosts)
    a, _, _ = _inputs(n, ghosts, n)
    for off in (0, 1):
        x = _Span(n + ghosts, off)
        _abi(pm, "pmg_vec_set", lay.handle, x.p, 2.5)
        assert _same(x.get(), np.full(n + ghosts, 2.5)), off
        x.assert_guards()
        x.put(a)
        _abi(pm, "pmg_vec_scale", lay.handle, x.p, -1.75)
        assert _same(x.get(), -1.75 * a), off
        x.assert_guards()


@pytest.mark.parametrize("ghosts", [0, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_copy_axpy_pointwise_mult_every_alignment(pm, n, ghosts):
    """copy, axpy and pointwise_mult act on the owned entries; every combination of aligned and 8-bytes-off operands
    (one operand off is enough for the scalar kernel) gives the same numbers and leaves ghosts, inputs and guards."""
    lay = pm.Layout(n, num_ghosts=ghosts)
    a, b, out0 = _inputs(n, ghosts, 7 * n + 1)
    alpha = -0.75
    ref_axpy, scale = alpha * a[:n] + b[:n], np.abs(alpha * a[:n]) + np.abs(b[:n])
    first = {}
    for o in itertools.product((0, 1), repeat=3):
        x, y = _Span(n + ghosts, o[1]).put(a), _Span(n + ghosts, o[2]).put(b)
        results = {}
        for op in ("copy", "axpy", "mult"):
            if op == "copy" and o[2]:
                continue
            r = _Span(n + ghosts, o[0]).put(out0)
            if op == "copy":
                _abi(pm, "pmg_vec_copy", lay.handle, r.p, x.p)
                got = r.get()
                assert _same(got[:n], a[:n]), o
            elif op == "axpy":
                _abi(pm, "pmg_vec_axpy", lay.handle, r.p, alpha, x.p, y.p)
                got = r.get()
                assert not np.isnan(got[:n]).any(), o
                _check("A axpy", (np.abs(got[:n] - ref_axpy) / scale).max(), TOL_VEC)
            else:
                _abi(pm, "pmg_vec_pointwise_mult", lay.handle, r.p, x.p, y.p)
                got = r.get()
                assert _same(got[:n], a[:n] * b[:n]), o
            assert _same(got[n:], out0[n:]), (op, o, "a ghost entry changed")
            r.assert_guards()
            results[op] = got[:n]
        assert _same(x.get(), a) and _same(y.get(), b), o
        x.assert_guards()
        y.assert_guards()
        if not first:
            first = results
        _note("A axpy aligned vs misaligned", np.abs(results["axpy"] - first["axpy"]).max())


@pytest.mark.parametrize("n", [1, 3, 64, 257, 513, 524289, 1048577])
def test_in_place_forms(pm, n):
    """The aliased calls the solvers and the drivers make: axpy(r, a, x, r), axpy(r, a, r, y), w = w .* y."""
    lay = pm.Layout(n)
    a, b, _ = _inputs(n, 0, 3 * n)
    for o in itertools.product((0, 1), repeat=2):
        r, x = _Span(n, o[0]).put(b), _Span(n, o[1]).put(a)
        _abi(pm, "pmg_vec_axpy", lay.handle, r.p, 0.37, x.p, r.p)
        _check("A axpy", (np.abs(r.get() - (0.37 * a + b)) / (np.abs(0.37 * a) + np.abs(b))).max(), TOL_VEC)
        r.put(a)
        y = _Span(n, o[1]).put(b)
        _abi(pm, "pmg_vec_axpy", lay.handle, r.p, -1.0, r.p, y.p)
        _check("A axpy", (np.abs(r.get() - (b - a)) / (np.abs(a) + np.abs(b))).max(), TOL_VEC)
        r.put(a)
        _abi(pm, "pmg_vec_pointwise_mult", lay.handle, r.p, r.p, y.p)
        assert _same(r.get(), a * b), o
        for s in (r, x, y):
            s.assert_guards()
        assert _same(x.get(), a) and _same(y.get(), b)


# ---------------------------------------------------------------------------------------------------------------------
# B. reductions
# ---------------------------------------------------------------------------------------------------------------------


def _f32(rng, n):
    """Doubles with 24 significant bits: the product of two is exact in FP64."""
    return rng.standard_normal(n).astype(np.float32).astype(np.float64)


def _dot(pm, lay, a, b):
    out = C.c_double(float("nan"))
    _abi(pm, "pmg_vec_inner_product", lay.handle, a.p, b.p, C.byref(out))
    return out.value


def _sqn(pm, lay, a):
    out = C.c_double(float("nan"))
    _abi(pm, "pmg_vec_squared_norm", lay.handle, a.p, C.byref(out))
    return out.value


def _norm(pm, lay, a, kind):
    out = C.c_double(float("nan"))
    _abi(pm, "pmg_vec_norm", lay.handle, a.p, {"l2": 0, "linf": 1}[kind], C.byref(out))
    return out.value


def _with_ghosts(v, ghosts):
    return np.concatenate([v, np.full(ghosts, GHOST)])


@pytest.mark.parametrize("ghosts", [0, 3])
@pytest.mark.parametrize("n", RED_LENGTHS)
def test_reductions_against_fsum(pm, n, ghosts):
    """Owned entries only (the ghosts hold 1e300), at every alignment of the two operands."""
    lay = pm.Layout(n, num_ghosts=ghosts)
    rng = np.random.default_rng(11 * n + ghosts)
    a, b = _f32(rng, n), _f32(rng, n)
    ab, aa = a * b, a * a
    ref_dot, sum_abs = math.fsum(ab.tolist()), math.fsum(np.abs(ab).tolist())
    ref_sq = math.fsum(aa.tolist())
    got = {}
    for oa, ob in itertools.product((0, 1), repeat=2):
        sa, sb = _Span(n + ghosts, oa).put(_with_ghosts(a, ghosts)), _Span(n + ghosts, ob).put(_with_ghosts(b, ghosts))
        d = _dot(pm, lay, sa, sb)
        _check("B inner_product", abs(d - ref_dot) / sum_abs, TOL_SUM)
        got.setdefault("dot", d)
        _note("B aligned vs misaligned", abs(d - got["dot"]) / sum_abs)
        if oa == ob:
            _check("B squared_norm", abs(_sqn(pm, lay, sa) - ref_sq) / ref_sq, TOL_SUM)
            _check("B norm l2", abs(_norm(pm, lay, sa, "l2") - math.sqrt(ref_sq)) / math.sqrt(ref_sq), TOL_SUM)
            assert _norm(pm, lay, sa, "linf") == np.abs(a).max()
        sa.assert_guards()
        sb.assert_guards()


@pytest.mark.parametrize("n", [513, 262145, 1048577])
def test_inner_product_with_heavy_cancellation(pm, n):
    """+-pairs of large products plus a small remainder: the sum is far below sum |a_i b_i|, and the bar is meant
    relative to the latter."""
    lay = pm.Layout(n)
    rng = np.random.default_rng(n)
    m = (3 * n) // 8
    big, c = _f32(rng, m) * 2.0**26, _f32(rng, m)
    rest = n - 2 * m
    a = np.concatenate([big, -big, _f32(rng, rest)])
    b = np.concatenate([c, c, _f32(rng, rest)])
    perm = rng.permutation(n)
    a, b = a[perm], b[perm]
    ab = a * b
    ref, sum_abs = math.fsum(ab.tolist()), math.fsum(np.abs(ab).tolist())
    assert abs(ref) < 1e-5 * sum_abs
    for oa, ob in itertools.product((0, 1), repeat=2):
        d = _dot(pm, lay, _Span(n, oa).put(a), _Span(n, ob).put(b))
        _check("B inner_product (cancellation)", abs(d - ref) / sum_abs, TOL_SUM)


@pytest.mark.parametrize("n", [1, 2, 3, 65, 257, 513, 262145, 1048577])
def test_linf_is_exact(pm, n):
    lay = pm.Layout(n)
    rng = np.random.default_rng(n)
    for off in (0, 1):
        assert _norm(pm, lay, _Span(n, off).put(np.zeros(n)), "linf") == 0.0
        # the largest magnitude is negative, in the first, a middle and the last (odd n: the tail) element
        for pos in sorted({0, n // 2, n - 1}):
            a = rng.uniform(-1.0, 1.0, n)
            a[pos] = -3.0 - pos / n
            assert _norm(pm, lay, _Span(n, off).put(a), "linf") == 3.0 + pos / n, (off, pos)
        a = -np.abs(rng.standard_normal(n)) - 0.5  # all negative
        assert _norm(pm, lay, _Span(n, off).put(a), "linf") == np.abs(a).max()


@pytest.mark.parametrize("n", [513, 262145, 3000001])
def test_reductions_repeat_bit_for_bit(pm, n):
    """two-stage deterministic reductions."""
    lay = pm.Layout(n)
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    for off in (0, 1):
        sa, sb = _Span(n, off).put(a), _Span(n, off).put(b)
        runs = [(_dot(pm, lay, sa, sb), _sqn(pm, lay, sa), _norm(pm, lay, sa, "l2"), _norm(pm, lay, sa, "linf"))
                for _ in range(20)]
        assert all(_same(r, runs[0]) for r in runs), off
        assert not np.isnan(runs[0]).any()


@pytest.mark.parametrize("n", [1, 3, 257, 262145, 1048577])
def test_a_nan_comes_out_of_every_reduction(pm, n):
    """A poisoned vector must not look finite to any norm (the check behind
    test_cg_reports_a_poisoned_right_hand_side reads one)."""
    lay = pm.Layout(n)
    rng = np.random.default_rng(n)
    b = rng.standard_normal(n)
    for off in (0, 1):
        sb = _Span(n, off).put(b)
        for pos in sorted({0, n // 2, n - 1}):
            a = rng.standard_normal(n)
            a[pos] = np.nan
            sa = _Span(n, off).put(a)
            assert math.isnan(_dot(pm, lay, sa, sb)), (off, pos)
            assert math.isnan(_dot(pm, lay, sb, sa)), (off, pos)
            assert math.isnan(_sqn(pm, lay, sa)), (off, pos)
            assert math.isnan(_norm(pm, lay, sa, "l2")), (off, pos)
            assert math.isnan(_norm(pm, lay, sa, "linf")), (off, pos)


# ---------------------------------------------------------------------------------------------------------------------
# C. the Chebyshev passes
# ---------------------------------------------------------------------------------------------------------------------

MESH = (4, 4, 8)  # even cell counts: every level has an odd number of dofs; degree 3 and 4 get several patches
HIERARCHIES = {"1-level": ((3,), True), "2-level-cell": ((1, 3), False), "2-level-patch": ((1, 3), True),
               "3-level-cell": ((1, 2, 4), False), "3-level-patch": ((1, 2, 4), True)}
PLANS = {"merged": None, "coloured": 0}


@functools.lru_cache(maxsize=None)
def _host_hierarchy(orders, numbering):
    """Host arrays and oracle objects of every level (they depend neither on k nor on the launch plan).  Dirichlet dofs:
    the face x = 0 only, so the corner (1, 1, 1) -- the last dof of the lexicographic numbering -- is an interior dof;
    "permuted" renumbers the dofs of every level at random, again with a free dof last."""
    import pmg_dolfinx_amd as pm
    from oracle import pmg_oracle as po

    part, flat = pm.BoxPartition(MESH, warp=warp), pm.BoxPartition(MESH)
    rng = np.random.default_rng(99)
    levels = []
    for P in orders:
        lv = part.level(P)
        nd = lv.ndofs
        bc = (flat.dof_coordinates(P)[:, 0] < 1e-12).astype(np.int8)
        perm = np.arange(nd)
        if numbering == "permuted":
            perm = rng.permutation(nd)  # old dof -> new dof
            j = int(np.nonzero(perm == nd - 1)[0][0])
            if bc[j]:
                f = int(np.nonzero(bc == 0)[0][nd // 3])
                perm[j], perm[f] = perm[f], perm[j]
        dofmap = perm[lv.dofmap].astype(np.int32)
        bcm = np.zeros(nd, np.int8)
        bcm[perm] = bc
        assert nd % 2 == 1 and bcm[-1] == 0 and bcm.sum() > 0
        A = po.Laplacian(P, 2.0, dofmap, part.xgeom, part.geom_dofmap, bcm)
        eig, _ = po.estimate_eig_range(A, nd)
        levels.append(dict(P=P, lv=lv, nd=nd, dofmap=dofmap, bc=bcm, A=A, eig=eig))
    interps = [po.Interpolator(c["P"], f["P"], c["dofmap"], f["dofmap"], c["nd"], f["nd"])
               for c, f in zip(levels[:-1], levels[1:])]
    b = rng.standard_normal(levels[-1]["nd"])
    b[levels[-1]["bc"].astype(bool)] = 0.0
    return dict(part=part, levels=levels, interps=interps, b=b)


def _oracle_cycle(H, k):
    from oracle import pmg_oracle as po

    sm = [po.Chebyshev(lv["eig"], k) for lv in H["levels"]]
    return po.MultigridPreconditioner([lv["A"] for lv in H["levels"]], sm, H["interps"], H["levels"][0]["bc"])


class _Device:
    """The library's objects for a host hierarchy."""

    def __init__(self, pm, H, k, patched, merge):
        part = H["part"]
        self.layouts, self.ops, self.smoothers, self.interps = [], [], [], []
        if merge is not None:
            pm.set_merge_threshold(merge)
        try:
            for lv in H["levels"]:
                lay = pm.Layout(lv["nd"])
                op = pm.MatFreeLaplacian(lv["P"], 2.0, lv["dofmap"], part.xgeom, part.geom_dofmap, lv["lv"].lcells,
                                         lv["lv"].bcells, lv["bc"], lay)
                op.compute_diag_inverse()
                sm = pm.Chebyshev(lay, lv["eig"])
                sm.set_max_iterations(k)
                self.layouts.append(lay)
                self.ops.append(op)
                self.smoothers.append(sm)
            for i, (c, f) in enumerate(zip(H["levels"][:-1], H["levels"][1:])):
                self.interps.append(pm.Interpolator(c["P"], f["P"], c["dofmap"], f["dofmap"], f["lv"].lcells,
                                                    f["lv"].bcells, self.layouts[i], self.layouts[i + 1],
                                                    fine_operator=self.ops[i + 1] if patched else None))
        finally:
            pm.set_merge_threshold(-1)
        launches = [op.launches_per_apply() for op in self.ops]
        if merge is None:
            assert all(n == 1 for n in launches), launches  # one atomic launch: the smoother clears q behind itself
        else:
            assert max(launches) > 1, launches
        self.mg = pm.MultigridPreconditioner(self.layouts, H["levels"][0]["bc"])
        self.mg.set_solvers(self.smoothers)
        self.mg.set_operators(self.ops)
        self.mg.set_interpolators(self.interps)

    def set_k(self, k):
        for sm in self.smoothers:
            sm.set_max_iterations(k)


def _three_cycles(pm, H, D, k, off_b=0, off_x=0):
    """Three cycles from x = 0 against the oracle (the first takes the zero-guess paths of the coarser levels, the
    later ones the non-zero paths); returns the iterates."""
    mgo = _oracle_cycle(H, k)
    lay, n = D.layouts[-1], H["levels"][-1]["nd"]
    sb, sx = _Span(n, off_b).put(H["b"]), _Span(n, off_x, fill=0.0)
    vb, vx = _on(pm, lay, sb), _on(pm, lay, sx)
    xo = np.zeros(n)
    out = []
    for cyc in range(3):
        rn = D.mg.apply(vb, vx, verbose=True)
        xo = mgo.apply(H["b"], xo, compute_rnorm=True)
        got = sx.get()
        _check("C cycle iterate", _relerr(got, xo), TOL_SOLVE)
        _check("C cycle residual norm", abs(rn - mgo.rnorm) / max(mgo.rnorm, 1e-30), TOL_RNORM)
        assert xo[-1] != 0.0  # the tail element carries a correction
        out.append(got)
    assert _same(sb.get(), H["b"])
    sb.assert_guards()
    sx.assert_guards()
    return out


@pytest.mark.parametrize("numbering", ["lexicographic", "permuted"])
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("hier", sorted(HIERARCHIES))
def test_chebyshev_degrees_on_every_hierarchy(pm, hier, k, plan, numbering):
    orders, patched = HIERARCHIES[hier]
    H = _host_hierarchy(orders, numbering)
    D = _Device(pm, H, k, patched, PLANS[plan])
    _three_cycles(pm, H, D, k)


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("hier", sorted(HIERARCHIES))
def test_zero_smoothing_steps(pm, hier, plan):
    """max_iter = 0 is accepted: from a zero guess the cycle returns zero, from any other guess the guess itself
    (every level's correction is zero); a smoother solve leaves x alone."""
    orders, patched = HIERARCHIES[hier]
    H = _host_hierarchy(orders, "lexicographic")
    D = _Device(pm, H, 2, patched, PLANS[plan])
    lay, n = D.layouts[-1], H["levels"][-1]["nd"]
    x0 = np.random.default_rng(4).standard_normal(n)
    for off in (0, 1):
        sb = _Span(n, off).put(H["b"])
        sx = _Span(n, off, fill=0.0)
        # a cycle with k = 2 first: the coarser levels then hold corrections that the zero-fill of the k = 0
        # smoothers has to clear (prolongated, they would change x)
        D.set_k(2)
        D.mg.apply(_on(pm, lay, sb), _on(pm, lay, sx))
        assert np.abs(sx.get()).max() > 0.0
        D.set_k(0)
        sx.view.fill_(0.0)
        D.mg.apply(_on(pm, lay, sb), _on(pm, lay, sx))
        assert np.array_equal(sx.get(), np.zeros(n))
        sx.put(x0)
        D.mg.apply(_on(pm, lay, sb), _on(pm, lay, sx))
        assert np.array_equal(sx.get(), x0)
        D.smoothers[-1].solve(D.ops[-1], _on(pm, lay, sx), _on(pm, lay, sb))
        assert np.array_equal(sx.get(), x0)
        sx.assert_guards()
        sb.assert_guards()


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("hier", ["1-level", "2-level-patch", "3-level-cell"])
def test_cycles_on_misaligned_caller_vectors(pm, hier, k, plan):
    """Right-hand side and iterate 8 bytes past a 16-byte boundary, both or one of them: every pass that touches them
    runs its scalar body over the whole level (see the file header for which functors that covers)."""
    orders, patched = HIERARCHIES[hier]
    H = _host_hierarchy(orders, "lexicographic")
    D = _Device(pm, H, k, patched, PLANS[plan])
    aligned = _three_cycles(pm, H, D, k)
    for off_b, off_x in ((1, 1), (1, 0), (0, 1)):
        got = _three_cycles(pm, H, D, k, off_b, off_x)
        _note("C aligned vs misaligned", max(_relerr(g, a) for g, a in zip(got, aligned)))


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_smoother_solve_on_misaligned_caller_vectors(pm, k, plan):
    """Chebyshev.solve (no residual, non-zero guess) on an odd level with an interior tail dof."""
    from oracle import pmg_oracle as po

    H = _host_hierarchy((3,), "permuted")
    D = _Device(pm, H, k, True, PLANS[plan])
    lv, lay = H["levels"][0], D.layouts[0]
    x0 = np.random.default_rng(k).standard_normal(lv["nd"])
    ref = po.Chebyshev(lv["eig"], k).solve(lv["A"], x0.copy(), H["b"])
    assert ref[-1] != x0[-1]
    first = None
    for off_b, off_x in itertools.product((0, 1), repeat=2):
        sb, sx = _Span(lv["nd"], off_b).put(H["b"]), _Span(lv["nd"], off_x).put(x0)
        D.smoothers[0].solve(D.ops[0], _on(pm, lay, sx), _on(pm, lay, sb))
        got = sx.get()
        _check("C smoother solve", _relerr(got, ref), TOL_SOLVE)
        first = got if first is None else first
        _note("C aligned vs misaligned", _relerr(got, first))
        sb.assert_guards()
        sx.assert_guards()


# ---- two ranks as two threads of this process: ghosted layouts (the set-up of tests/test_gpu_distributed.py) ----


class _ThreadWorld:
    def __init__(self, n):
        import threading

        self.n = n
        self.barrier = threading.Barrier(n)
        self.layouts = [dict() for _ in range(n)]
        self.slots = [None] * n

    def wait(self):
        self.barrier.wait(timeout=240)


class _ThreadComm:
    native = None
    staged = False
    distributed = True

    def __init__(self, world, rank):
        self.W, self.rank, self.world = world, rank, world.n
        self._count = 0

    def register(self, layout):  # layouts are created in the same order on every rank
        layout._tid = self._count
        self.W.layouts[self.rank][self._count] = layout
        self._count += 1

    def exchange(self, L, phase):
        st = torch.cuda.current_stream()
        W = self.W
        if phase in (0, 2):
            fwd = phase == 0
            L._ev_packed = torch.cuda.Event()
            L._ev_packed.record(st)
            W.wait()
            off = 0
            for i, nb in enumerate(L.neighbors):
                peer = W.layouts[nb][L._tid]
                cnt = (L.recv_counts if fwd else L.send_counts)[i]
                j = peer.neighbors.index(self.rank)
                pc = peer.send_counts if fwd else peer.recv_counts
                assert pc[j] == cnt, "the two sides of a halo plan disagree"
                po_ = sum(pc[:j])
                st.wait_event(peer._ev_packed)
                src = (peer.send_buffer if fwd else peer.recv_buffer)[po_: po_ + cnt]
                dst = (L.recv_buffer if fwd else L.send_buffer)[off: off + cnt]
                dst.copy_(src)
                off += cnt
            L._ev_copied = torch.cuda.Event()
            L._ev_copied.record(st)
        else:
            W.wait()
            for nb in L.neighbors:
                st.wait_event(W.layouts[nb][L._tid]._ev_copied)

    def allreduce(self, L, host, op):
        W = self.W
        W.slots[self.rank] = host.copy()
        W.wait()
        vals = np.stack(W.slots)
        tot = vals.max(axis=0) if op == "max" else vals.sum(axis=0)
        W.wait()
        host[:] = tot


CG_CASES = [("diagonal", 3), ("vcycle", 1), ("vcycle", 2), ("vcycle", 4), ("flexible", 2)]


def _oracle_cg(A, b, precond, flexible, max_iter, rtol):
    from oracle import pmg_oracle as po

    ocg = po.CGSolver()
    ocg.set_max_iterations(max_iter)
    ocg.set_tolerance(rtol)
    ocg.store_coefficients(True)
    xo = np.zeros_like(b)
    its = ocg.solve(A, xo, b, precond=precond, flexible=flexible)
    return its, np.array(ocg.alphas), np.array(ocg.betas), xo


def _device_cg(pm, layout, op, mg, kind, vx, vb, max_iter, rtol):
    cg = pm.CGSolver(layout)
    cg.set_max_iterations(max_iter)
    cg.set_tolerance(rtol)
    cg.store_coefficients(True)
    cg.set_flexible(kind == "flexible")
    its = cg.solve(op, vx, vb, preconditioner=None if kind == "diagonal" else mg)
    return its, cg.alphas(), cg.betas()


def _cg_limits(kind):
    return (25, 1e-6) if kind == "diagonal" else (40, 1e-8)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_two_ranks_with_ghosts(pm, k):
    """proc_dims (1, 1, 2), two ranks as threads, Chebyshev degrees other than 3: the iterate's ghosts absorb every
    correction (track_ghosts, launch_add on the ghost range, which starts at an arbitrary offset), ThenClearF runs
    over more entries than the smoother owns; three cycles and the three CG variants against the single-domain
    oracle, on aligned and on misaligned caller vectors."""
    import threading

    from oracle import pmg_oracle as po

    n, dims, orders, world = (4, 4, 8), (1, 1, 2), (1, 2, 4), 2
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=k, warp=warp)
    W = _ThreadWorld(world)
    res, errors, shared = [None] * world, [], {}

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                H = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=k, proc_dims=dims, rank=rank, size=world,
                                        warp=warp, comm=_ThreadComm(W, rank))
                lv, lay, op = H.levels[-1], H.layouts[-1], H.operators[-1]
                assert all(l.num_ghosts > 0 for l in H.levels)
                own = lv.local_to_global[: lv.size_local]
                if rank == 0:  # the oracle, with this hierarchy's smoother bounds
                    for s_, e in zip(sm, H.eig_ranges):
                        s_.eig_range = e
                    xo = np.zeros_like(b)
                    shared["cycles"] = []
                    for _ in range(3):
                        xo = mg.apply(b, xo, compute_rnorm=True)
                        shared["cycles"].append((xo.copy(), mg.rnorm))
                    vc = lambda r: mg.apply(r, np.zeros_like(r))  # noqa: E731
                    shared["cg"] = {kind: _oracle_cg(ops[-1], b, None if kind == "diagonal" else vc,
                                                     kind == "flexible", *_cg_limits(kind))
                                    for kind in ("diagonal", "vcycle", "flexible")}
                W.wait()
                out = {"cycle": [], "rnorm": [], "cg": [], "guards": True, "vs_aligned": 0.0}
                bl = np.zeros(lv.ndofs)
                bl[: lv.size_local] = b[own]
                for off in (0, 1):
                    sb, sx = _Span(lv.ndofs, off).put(bl), _Span(lv.ndofs, off, fill=0.0)
                    vb, vx = _on(pm, lay, sb), _on(pm, lay, sx)
                    for c in range(3):
                        rn = H.mg.apply(vb, vx, verbose=True)
                        ref, rno = shared["cycles"][c]
                        got = sx.get()[: lv.size_local]
                        out["cycle"].append(float(np.abs(got - ref[own]).max() / np.abs(ref).max()))
                        out["rnorm"].append(abs(rn - rno) / rno)
                        if off == 0:
                            out.setdefault("aligned", []).append(got)
                        else:
                            out["vs_aligned"] = max(out["vs_aligned"],
                                                    float(np.abs(got - out["aligned"][c]).max() / np.abs(ref).max()))
                    for kind in ("diagonal", "vcycle", "flexible"):
                        sx.view.fill_(0.0)
                        its, al, be = _device_cg(pm, lay, op, H.mg, kind, vx, vb, *_cg_limits(kind))
                        oits, oal, obe, xo = shared["cg"][kind]
                        got = sx.get()[: lv.size_local]
                        out["cg"].append((kind, off, its, oits, len(al) == len(oal) and len(be) == len(obe),
                                          float(np.abs(al / oal[: len(al)] - 1).max()) if len(al) else 0.0,
                                          float(np.abs(be / obe[: len(be)] - 1).max()) if len(be) else 0.0,
                                          float(np.abs(got - xo[own]).max() / np.abs(xo).max())))
                    torch.cuda.current_stream().synchronize()
                    for s_ in (sb, sx):
                        s_.assert_guards()
                res[rank] = out
        except BaseException:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            W.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, "\n".join(f"rank {r}:\n{tb}" for r, tb in errors)
    assert all(r is not None for r in res)
    for out in res:
        _check("C cycle iterate (two ranks)", max(out["cycle"]), TOL_SOLVE)
        _check("C cycle residual norm (two ranks)", max(out["rnorm"]), TOL_RNORM)
        _note("C aligned vs misaligned", out["vs_aligned"])
        for kind, off, its, oits, same_len, ea, eb, ex in out["cg"]:
            assert its == oits and same_len, (kind, off, its, oits)
            _check("D alpha (two ranks)", ea, TOL_CG)
            _check("D beta (two ranks)", eb, TOL_CG)
            _check("D iterate (two ranks)", ex, TOL_CG)


# ---- the streaming threshold: a level streams (non-temporal loads and stores) from 4 << 20 = 4 194 304 dofs ----

# 161^3 = 4 173 281 (below, odd), 162^3 = 4 251 528 (above, even), 163^3 = 4 330 747 (above, odd)
STREAMING = {"below-odd": (1, 160, 161**3), "above-even": (1, 161, 162**3), "above-odd": (2, 81, 163**3)}


@functools.lru_cache(maxsize=None)
def _lmax(P):
    """An upper eigenvalue bound of the Jacobi-scaled degree-P operator (from a small mesh; it hardly moves with h,
    and any value above the spectrum gives a valid smoother to compare)."""
    from oracle import pmg_oracle as po

    m = po.BoxMesh(6)
    A = po.Laplacian(P, 2.0, m.dofmap(P), m.xgeom, m.geom_dofmap, m.boundary_marker(P))
    return 1.15 * po.estimate_eig_range(A, A.ndofs)[0][1]


@pytest.mark.parametrize("size", sorted(STREAMING))
def test_smoother_solve_around_the_streaming_threshold(pm, size):
    """A single-level smoother solve at k = 1, 2, 4 against the C oracle, aligned and misaligned once each."""
    from oracle import c_oracle as co

    P, cells, ndofs = STREAMING[size]
    part = pm.BoxPartition(cells)
    lv = part.level(P)
    assert lv.ndofs == ndofs and (ndofs >= 4 << 20) == (size != "below-odd")
    lay = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker, lay)
    op.compute_diag_inverse()
    cl = co.CLevel(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    rng = np.random.default_rng(ndofs)
    x0, b = rng.standard_normal(ndofs), rng.standard_normal(ndofs)
    sm = pm.Chebyshev(lay, (0.1 * _lmax(P), _lmax(P)))
    for k, off in ((1, 0), (2, 1), (4, 0), (1, 1), (4, 1), (2, 0)):
        sm.set_max_iterations(k)
        sb, sx = _Span(ndofs, off).put(b), _Span(ndofs, off).put(x0)
        sm.solve(op, _on(pm, lay, sx), _on(pm, lay, sb))
        ref, _ = cl.cheb_solve(_lmax(P), k, x0.copy(), b, need_r=False, x_zero=False)
        _check(f"C streaming smoother solve ({size})", _relerr(sx.get(), ref), TOL_SOLVE)
        sb.assert_guards()
        sx.assert_guards()


@pytest.mark.parametrize("patched", [False, True], ids=["cell", "patch"])
def test_two_level_cycle_above_the_streaming_threshold(pm, patched):
    """Degree 2 on 81^3 cells (163^3 dofs, odd, streaming) over degree 1: three cycles from x = 0 at k = 1, 2, 4
    against the C oracle -- the residual kernels (ChebLastF, ChebResidualF) and the first steps in their streaming
    forms; the cell form on misaligned, the patch form on aligned caller vectors."""
    from oracle import c_oracle as co

    cells, orders = 81, (1, 2)
    part = pm.BoxPartition(cells)
    lvs = [part.level(P) for P in orders]
    assert lvs[-1].ndofs == 163**3 >= 4 << 20
    lays = [pm.make_layout(lv) for lv in lvs]
    ops = []
    for P, lv, lay in zip(orders, lvs, lays):
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 lay)
        op.compute_diag_inverse()
        ops.append(op)
    lmax = [_lmax(P) for P in orders]
    sms = [pm.Chebyshev(lay, (0.1 * lm, lm)) for lay, lm in zip(lays, lmax)]
    ip = pm.Interpolator(1, 2, lvs[0].dofmap, lvs[1].dofmap, lvs[1].lcells, lvs[1].bcells, lays[0], lays[1],
                         fine_operator=ops[1] if patched else None)
    mg = pm.MultigridPreconditioner(lays, lvs[0].bc_marker)
    mg.set_solvers(sms)
    mg.set_operators(ops)
    mg.set_interpolators([ip])
    cl = [co.CLevel(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker) for P, lv in zip(orders, lvs)]
    ci = [co.CInterp(cl[0], cl[1])]
    n = lvs[-1].ndofs
    b = np.random.default_rng(5).standard_normal(n)
    b[lvs[-1].bc_marker.astype(bool)] = 0.0
    off = 0 if patched else 1
    for k in (1, 2, 4):
        for sm in sms:
            sm.set_max_iterations(k)
        cm = co.CMultigrid(cl, ci, lmax, k)
        sb, sx = _Span(n, off).put(b), _Span(n, off, fill=0.0)
        xo = np.zeros(n)
        for cyc in range(3):
            mg.apply(_on(pm, lays[-1], sb), _on(pm, lays[-1], sx))
            cm.apply(b, xo)
            _check("C streaming two-level cycle", _relerr(sx.get(), xo), TOL_SOLVE)
        sb.assert_guards()
        sx.assert_guards()


# ---------------------------------------------------------------------------------------------------------------------
# D. the CG passes
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,k", CG_CASES)
def test_cg_passes(pm, kind, k):
    """CgUpdateF (diagonal), CgUpdate2F (V-cycle) and CgDirectionF with d_sub (flexible) on an odd level whose tail dof
    is interior, x and b aligned and 8 bytes off.  As a preconditioner the cycle starts from a zero guess on EVERY
    level: the first-step and one-step kernels of the finest level run here."""
    H = _host_hierarchy((1, 2, 4), "lexicographic")
    D = _Device(pm, H, k, True, None)
    lv, lay = H["levels"][-1], D.layouts[-1]
    mgo = _oracle_cycle(H, k)
    if kind == "flexible":
        # a preconditioner that is not a fixed linear operator -- four CG steps on the coarsest level, as
        # test_flexible_pcg_with_krylov_coarse_solver -- so that r_new . z_old, the d_sub term, is not rounding noise
        from oracle import pmg_oracle as po

        ccg = pm.CGSolver(D.layouts[0])
        ccg.set_max_iterations(4)
        ccg.set_tolerance(0.0)
        D.mg.set_coarse_solver(ccg)

        def coarse(u0, b0):
            c = po.CGSolver()
            c.set_max_iterations(4)
            c.set_tolerance(0.0)
            u0[:] = 0.0
            c.solve(H["levels"][0]["A"], u0, b0)

        mgo.coarse = coarse
    vc = lambda r: mgo.apply(r, np.zeros_like(r))  # noqa: E731
    max_iter, rtol = _cg_limits(kind)
    oits, oal, obe, xo = _oracle_cg(lv["A"], H["b"], None if kind == "diagonal" else vc, kind == "flexible", max_iter,
                                    rtol)
    assert oits > 2 and xo[-1] != 0.0
    first = None
    for off_b, off_x in ((0, 0), (1, 1), (0, 1), (1, 0)):
        sb, sx = _Span(lv["nd"], off_b).put(H["b"]), _Span(lv["nd"], off_x, fill=0.0)
        its, al, be = _device_cg(pm, lay, D.ops[-1], D.mg, kind, _on(pm, lay, sx), _on(pm, lay, sb), max_iter, rtol)
        assert its == oits and len(al) == len(oal) and len(be) == len(obe), (its, oits)
        _check("D alpha", np.abs(al / oal - 1).max(), TOL_CG)
        _check("D beta", np.abs(be / obe - 1).max(), TOL_CG)
        got = sx.get()
        _check("D iterate", _relerr(got, xo), TOL_CG)
        first = got if first is None else first
        _note("D aligned vs misaligned", _relerr(got, first))
        assert _same(sb.get(), H["b"])
        sb.assert_guards()
        sx.assert_guards()
