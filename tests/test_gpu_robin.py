"""The Robin boundary term (pmg_laplacian_set_robin): K grad u . n + alpha u = g on listed facets puts the diagonal
face mass d_R[dof] = sum of w1[i] w1[j] |dS| alpha over the facet points on the dof onto the operator, beside the
reaction term's d_sigma: y = A x + (d_sigma + d_R) x on unmarked rows, y = x on marked ones.

The CPU truth is tests/robin_reference.py -- the oracle's operator plus the two vectors, pinned from first principles
in tests/test_robin_abi.py.  alpha is random in [0, 4] per facet point with about a fifth exactly 0
(``rb.random_alpha``), and the Dirichlet marker is restricted to the face x = 0, so the dofs of the other five faces are
unmarked and carry the term.

How the errors are measured (tests/test_gpu_reaction.py's measure): the marked rows must equal x exactly, and the
relative max error is taken over the unmarked rows alone, < 1e-12 per apply in FP64, < 1e-10 after a V-cycle or a
Chebyshev solve, NOISE = 1e-14 between two runs on the same bits.  The per-cell kappa is drawn from
[0.5, 1.5] * 0.5 / P^2 (``_kappa``), which puts the term at several per cent of a boundary row, and every parity test
also asserts that the reference WITHOUT d_R is more than 1e-2 away over the unmarked rows that lie on a listed facet
(interior rows do not see the term).  FP32: the bounds of tests/test_gpu_reaction.py (twice the FP32 error of the same
operator without the term, itself < 1e-5) and tests/test_gpu_mixed_precision.py (1e-4 for a cycle against the FP64
oracle, 1e-6 between graph replay and eager)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as bd  # noqa: E402
import reaction_reference as rr  # noqa: E402
import robin_reference as rb  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NOISE = 1e-14
FULL_PATCHES = [(1, (8, 8, 16)), (2, (4, 4, 16)), (3, (4, 4, 8)), (4, (4, 4, 8)), (5, (4, 4, 14)), (6, (2, 4, 8)),
                (7, (2, 2, 6)), (8, (2, 2, 6))]
CUT_SHORT = [(2, (3, 3, 3), "twist"), (3, (3, 3, 3), "warp"), (4, (3, 3, 3), "twist")]
MAPS = {None: None, "twist": bd.twist, "warp": bd.warp}


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


def _x0_face(c):
    return np.abs(c[:, 0]) < 1e-12


class Case:
    """An operator without the term yet, on a marker restricted to x = 0 (or ``bc``), and the test's coefficients."""

    def __init__(self, pm, n, P, wf, seed, coloured=False, bc=None, node_order="ascending", kappa=None):
        self.pm, self.P, self.n = pm, P, n
        self.part = pm.BoxPartition(n, warp=MAPS.get(wf, wf))
        self.lv = self.part.level(P)
        self.layout = pm.make_layout(self.lv)
        self.bc = rb.one_face_marker(self.lv.bc_marker, self.part.dof_coordinates(P)) if bc is None else bc
        self.kappa = _kappa(P, self.part.ncells, 300 + seed) if kappa is None else kappa
        self.cells, self.facets = self.part.exterior_facets()
        self.alpha = rb.random_alpha(self.cells.size, (P + 1) ** 2, 700 + seed)
        self.sigma = rr.random_sigma(self.part.ncells, 500 + seed)
        self.coloured, self.node_order = coloured, node_order
        self.op = self.operator()

    def operator(self):
        pm, lv, part = self.pm, self.lv, self.part
        dm = lv.dofmap
        if self.node_order != "ascending":
            dm = pm.dofmap_in_node_order(lv.dofmap, pm.basix_node_permutation(self.P))
        try:
            if self.coloured:
                pm.set_merge_threshold(0)
            return pm.MatFreeLaplacian(self.P, self.kappa, dm, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                       self.bc, self.layout, node_order=self.node_order)
        finally:
            if self.coloured:
                pm.set_merge_threshold(-1)

    def set(self, op=None, alpha=None):
        (self.op if op is None else op).set_robin(self.cells, self.facets, self.alpha if alpha is None else alpha)

    def oracle(self, alpha=None, sigma=None, robin=True):
        a = self.alpha if alpha is None else alpha
        if not robin:
            a = np.zeros_like(self.alpha)
        return rb.laplacian(self.part, self.P, self.kappa, self.lv.dofmap, self.bc, self.cells, self.facets, a, sigma)

    def on_facets(self, cells=None, facets=None):
        """The unmarked rows that lie on a listed facet."""
        cells, facets = (self.cells, self.facets) if cells is None else (cells, facets)
        on = np.zeros(self.lv.ndofs, dtype=bool)
        on[bd.facet_dofs(self.P, self.lv.dofmap, cells, facets).ravel()] = True
        return on & ~self.bc.astype(bool)

    def apply(self, u, op=None, fill=7.0):
        x, y = _vec(self.pm, self.layout, u), self.pm.Vector(self.layout)
        y.set(fill)
        (self.op if op is None else op)(x, y)
        return y

    def diag(self, op=None):
        d = self.pm.Vector(self.layout)
        (self.op if op is None else op).get_diag_inverse(d)
        return d.data_copy()

    def check_apply(self, A, u, op=None, tol=1e-12):
        got = self.apply(u, op).data_copy()
        err = _rows(got, A.apply(u), u, self.bc)
        assert err < tol, err
        return err

    def away(self, A, u, mask=None):
        """How far the reference without d_R is, over the unmarked rows on a listed facet."""
        mask = self.on_facets() if mask is None else mask
        ref = A.apply(u)
        without = ref - A.d_R * u
        return _relerr(without[mask], ref[mask])


def _tiny_kappa_vector(c, op=None):
    """d_R read through the operator: with kappa -> tiny, A x is nothing beside it, and y = d_R .* 1 on unmarked
    rows."""
    return c.apply(np.ones(c.lv.ndofs), op).data_copy()


# ---- 1. the vector itself ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", range(1, 9))
def test_robin_vector_all_degrees(pm, P):
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    c = Case(pm, n, P, "twist", P, kappa=np.full(pm.BoxPartition(n).ncells, 1e-30))
    assert not c.op.has_robin()
    c.set()
    assert c.op.has_robin() and not c.op.has_reaction()
    want = rb.robin_vector(c.part, P, c.lv.dofmap, c.cells, c.facets, c.alpha, c.bc)
    got = _tiny_kappa_vector(c)
    free = ~c.bc.astype(bool)
    err = _relerr(got[free], want[free])
    print(f"P = {P}: d_R through a unit-vector apply {err:.3e}; {int((want > 0).sum())} dofs carry the term")
    assert np.array_equal(got[~free], np.ones(int((~free).sum())))  # marked rows: y = x
    assert err < 1e-12
    assert (want[c.on_facets()] > 0).mean() > 0.5 and np.all(want[~c.on_facets()] == 0)
    # a device tensor is taken as it is
    c.set(alpha=torch.from_numpy(c.alpha).cuda())
    assert _relerr(_tiny_kappa_vector(c)[free], want[free]) < 1e-12


# ---- 2. every local facet alone ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("facet", range(6))
def test_each_local_facet_alone(pm, facet):
    P, n = 3, (2, 3, 2)
    nomark = np.zeros(pm.BoxPartition(n).level(P).ndofs, dtype=np.int8)
    c = Case(pm, n, P, "twist", 10 + facet, bc=nomark, kappa=np.full(12, 1e-30))
    on = c.facets == facet
    cells, facets, alpha = c.cells[on], c.facets[on], c.alpha[on]
    assert cells.size == {0: 6, 1: 6, 2: 4, 3: 4, 4: 6, 5: 6}[facet]
    c.op.set_robin(cells, facets, alpha)
    want = rb.robin_vector(c.part, P, c.lv.dofmap, cells, facets, alpha, nomark)
    got = _tiny_kappa_vector(c)
    assert _relerr(got, want) < 1e-12
    other = rb.robin_vector(c.part, P, c.lv.dofmap, cells, facets ^ 1, alpha, nomark)  # the opposite face
    assert _relerr(other, want) > 1e-2
    mask = c.on_facets(cells, facets)
    assert np.all(want[~mask] == 0) and (want[mask] > 0).mean() > 0.5


# ---- 3. basix node order: the facet points stay ascending -------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 4])
def test_basix_node_order(pm, P):
    c = Case(pm, (3, 2, 4), P, "twist", 20 + P, node_order="basix")
    c.set()
    A = c.oracle()
    u = np.random.default_rng(20 + P).standard_normal(c.lv.ndofs)
    c.check_apply(A, u)
    assert c.away(A, u) > 1e-2
    c.op.compute_diag_inverse()
    assert _relerr(c.diag(), A.diag_inverse()) < 1e-12


# ---- 4. FP64 apply ----------------------------------------------------------------------------------------------------


def _fp64_modes(pm, c, A, u):
    from pmg_dolfinx_amd import _lib

    e = [c.check_apply(A, u)]
    y = c.apply(u, fill=-3.0)
    c.op(_vec(pm, c.layout, u), y)  # a second application into the same y
    assert _rows(y.data_copy(), A.apply(u), u, c.bc) < 1e-12
    if c.op.is_affine():
        c.op.set_geometry_mode("affine")
        e.append(c.check_apply(A, u))
        c.set()  # set again while in affine mode
        e.append(c.check_apply(A, u))
        c.op.set_geometry_mode("stored")
    _lib.call("pmg_laplacian_set_geometry_batch", c.op.handle, 8)  # the Python class refuses batching: the C entry
    e.append(c.check_apply(A, u))
    c.op.compute_diag_inverse()
    assert _relerr(c.diag(), A.diag_inverse()) < 1e-12
    _lib.call("pmg_laplacian_set_geometry_batch", c.op.handle, 0)
    e.append(c.check_apply(A, u))
    return max(e)


@pytest.mark.parametrize("coloured", [False, True], ids=["merged", "coloured"])
@pytest.mark.parametrize("P,n", FULL_PATCHES)
def test_fp64_apply_full_patches(pm, P, n, coloured):
    c = Case(pm, n, P, None, 30 + P, coloured)
    assert c.op.is_affine()
    c.set()
    A = c.oracle()
    u = np.random.default_rng(30 + P).standard_normal(c.lv.ndofs)
    err, away = _fp64_modes(pm, c, A, u), c.away(A, u)
    print(f"P = {P} {n} {'coloured' if coloured else 'merged'}: worst apply error {err:.3e}; without d_R {away:.3e}")
    assert away > 1e-2


@pytest.mark.parametrize("coloured", [False, True], ids=["merged", "coloured"])
@pytest.mark.parametrize("P,n,wf", CUT_SHORT)
def test_fp64_apply_cut_short_and_mapped(pm, P, n, wf, coloured):
    c = Case(pm, n, P, wf, 40 + P, coloured)
    assert c.op.is_affine() == (wf == "warp")  # (that map shears each cell; the twisted cells are not parallelepipeds)
    c.set()
    A = c.oracle()
    u = np.random.default_rng(40 + P).standard_normal(c.lv.ndofs)
    _fp64_modes(pm, c, A, u)
    assert c.away(A, u) > 1e-2


# ---- 5. FP32 apply ----------------------------------------------------------------------------------------------------


def _fp32_vs_fp64(pm, c, op, u32):
    x = torch.from_numpy(u32).cuda()
    y = torch.full_like(x, 7.0)
    op.apply_fp32(x, y)
    torch.cuda.synchronize()
    ref = c.apply(u32.astype(np.float64), op).data_copy()
    return _rows(y.cpu().numpy().astype(np.float64), ref, u32.astype(np.float64), c.bc), ref


@pytest.mark.parametrize("coloured", [False, True], ids=["merged", "coloured"])
@pytest.mark.parametrize("P,n", FULL_PATCHES)
def test_fp32_apply(pm, P, n, coloured):
    """apply_fp32 against the FP64 apply of the same operator, itself checked against the reference.  The bound is
    tests/test_gpu_reaction.py's: the error measured on the same operator without the term, times 2 (the term adds one
    rounding of d to float and one product per dof).  The float apply reads the float tensor in either geometry mode;
    in batched-geometry mode the library refuses FP32 with or without the term, and that is what is asserted."""
    from pmg_dolfinx_amd import _lib

    c = Case(pm, n, P, None, 50 + P, coloured)
    u32 = np.random.default_rng(50 + P).standard_normal(c.lv.ndofs).astype(np.float32)
    u = u32.astype(np.float64)
    e0, y_plain = _fp32_vs_fp64(pm, c, c.op, u32)  # builds the float tensor
    assert 0 < e0 < 1e-5
    early = c.operator()
    c.set(early)  # before the first FP32 use
    c.set()       # the float tensor exists already
    A = c.oracle()
    c.check_apply(A, u)
    e1, y_early = _fp32_vs_fp64(pm, c, early, u32)
    e2, y_late = _fp32_vs_fp64(pm, c, c.op, u32)
    c.op.set_geometry_mode("affine")
    e3, _ = _fp32_vs_fp64(pm, c, c.op, u32)
    c.op.set_geometry_mode("stored")
    mask = c.on_facets()
    print(f"P = {P} {'coloured' if coloured else 'merged'}: fp32 vs fp64 without the term {e0:.3e}; set first {e1:.3e}, "
          f"set after FP32 use {e2:.3e}, affine mode {e3:.3e}")
    assert _relerr(y_late[mask], y_plain[mask]) > 1e-2
    assert c.away(A, u) > 1e-2
    assert max(e1, e2, e3) <= 2 * e0
    assert _relerr(y_late, y_early) < 1e-13
    _lib.call("pmg_laplacian_set_geometry_batch", c.op.handle, 8)
    x = torch.from_numpy(u32).cuda()
    with pytest.raises(pm._lib.PmgError, match="resident geometry"):
        c.op.apply_fp32(x, torch.empty_like(x))
    _lib.call("pmg_laplacian_set_geometry_batch", c.op.handle, 0)
    e4, _ = _fp32_vs_fp64(pm, c, c.op, u32)
    assert e4 <= 2 * e0


# ---- 6. two terms, set and removed independently ----------------------------------------------------------------------


def _order_free_boundary_vector(c, seed):
    """(u, rows): a vector that sees the boundary, and the rows on which its apply has one bit pattern whatever order
    the cell sums arrive in.  u is non-zero on the unmarked face-interior nodes of the exterior facets only; each of
    those belongs to one cell, so the output entry on such a row is d * x plus that one cell's product.  Bit identity
    is asserted on these rows alone."""
    P, nd = c.P, c.P + 1
    u = np.zeros(c.lv.ndofs)
    rows = []
    rng = np.random.default_rng(seed)
    for cell, lf in zip(c.cells, c.facets):
        t, ii, jj = bd.facet_nodes_axes(P, int(lf))
        inner = t[(ii > 0) & (ii < P) & (jj > 0) & (jj < P)]
        rows.append(c.lv.dofmap[cell][inner])
    rows = np.unique(np.concatenate(rows))
    rows = rows[~c.bc.astype(bool)[rows]]
    u[rows] = rng.standard_normal(rows.size)
    return u, rows


@pytest.mark.parametrize("P,n,coloured", [(4, (4, 4, 8), True), (2, (5, 4, 3), False)])
def test_robin_and_reaction_in_both_orders(pm, P, n, coloured):
    c = Case(pm, n, P, "twist", 60 + P, coloured)
    u = np.random.default_rng(60 + P).standard_normal(c.lv.ndofs).astype(np.float32).astype(np.float64)
    A_r, A_s, A_rs = c.oracle(), c.oracle(sigma=c.sigma, robin=False), c.oracle(sigma=c.sigma)
    only_r, only_s, fresh = c.operator(), c.operator(), c.operator()
    c.set(only_r)
    only_s.set_reaction(c.sigma)
    for op in (only_r, only_s, fresh):
        op.compute_diag_inverse()
    c.check_apply(A_r, u, only_r)
    c.check_apply(A_s, u, only_s)
    assert (only_r.has_robin(), only_r.has_reaction()) == (True, False)
    assert (only_s.has_robin(), only_s.has_reaction()) == (False, True)
    ub, rows = _order_free_boundary_vector(c, 61)
    assert rows.size > 10
    x32 = torch.from_numpy(u.astype(np.float32)).cuda()

    def fp32(op):
        y = torch.full_like(x32, 7.0)
        op.apply_fp32(x32, y)
        return y

    for robin_first in (True, False):
        op = c.operator()
        op.compute_diag_inverse()
        fp32(op)  # the float tensor exists from the start
        if robin_first:
            c.set(op)
            c.check_apply(A_r, u, op)
            op.set_reaction(c.sigma)
        else:
            op.set_reaction(c.sigma)
            c.check_apply(A_s, u, op)
            c.set(op)
        assert op.has_robin() and op.has_reaction()
        c.check_apply(A_rs, u, op)
        assert c.away(A_rs, u) > 1e-2
        assert _relerr(c.diag(op), A_rs.diag_inverse()) < 1e-12  # the inverse diagonal followed both sets
        e32 = _rows(fp32(op).cpu().numpy().astype(np.float64), A_rs.apply(u), u, c.bc)
        assert e32 < 1e-5
        # remove one: the other alone remains, as on an operator that only ever had that one
        if robin_first:
            op.set_reaction(None)
            left, A_left = only_r, A_r
        else:
            op.set_robin(None, None, None)
            left, A_left = only_s, A_s
        assert (op.has_robin(), op.has_reaction()) == (robin_first, not robin_first)
        c.check_apply(A_left, u, op)
        assert _relerr(c.apply(u, op).data_copy(), c.apply(u, left).data_copy()) < NOISE
        assert _relerr(c.diag(op), c.diag(left)) < NOISE
        assert _relerr(fp32(op).cpu().numpy(), fp32(left).cpu().numpy()) < 1e-6
        # remove both: the operator without a term, bit for bit where the sums have one order
        if robin_first:
            op.set_robin(c.cells[:0], c.facets[:0], None)
        else:
            op.set_reaction(None)
        assert not op.has_robin() and not op.has_reaction()
        assert torch.equal(c.apply(ub, op).data[rows], c.apply(ub, fresh).data[rows])
        assert _relerr(c.apply(u, op).data_copy(), c.apply(u, fresh).data_copy()) < NOISE
        assert _relerr(c.diag(op), c.diag(fresh)) < NOISE
        xb = torch.from_numpy(ub.astype(np.float32)).cuda()
        y_op, y_fresh = torch.full_like(xb, 7.0), torch.full_like(xb, 7.0)
        op.apply_fp32(xb, y_op)
        fresh.apply_fp32(xb, y_fresh)
        assert torch.equal(y_op[rows], y_fresh[rows])
        op.set_robin(None, None, None)  # nothing to remove: no error
    # exact copies: the Robin component alone is the same vector whether sigma was ever there or not (it is rebuilt
    # by atomics per set, so two sets agree to NOISE; a removal of sigma copies it bit for bit)
    op = c.operator()
    c.set(op)
    before = c.apply(ub, op).data.clone()
    op.set_reaction(c.sigma)
    assert not torch.equal(c.apply(ub, op).data[rows], before[rows])
    op.set_reaction(None)
    assert torch.equal(c.apply(ub, op).data[rows], before[rows])
    # a diagonal installed by the caller is not overwritten
    mine = np.random.default_rng(5).uniform(0.1, 1.0, c.lv.ndofs)
    op.set_diag_inverse(_vec(pm, c.layout, mine))
    c.set(op)
    assert np.array_equal(c.diag(op), mine)


# ---- 7. fused residual restriction ------------------------------------------------------------------------------------


@pytest.mark.parametrize("pf,pc,n", [(2, 1, (4, 4, 16)), (3, 1, (4, 4, 8)), (4, 2, (4, 4, 16)), (6, 3, (2, 4, 8))])
def test_fused_residual_restriction(pm, pf, pc, n):
    from oracle import pmg_oracle as po

    c = Case(pm, n, pf, "warp", 70 + pf)
    lc = c.part.level(pc)
    Lc = pm.make_layout(lc)
    c.set()
    c.op.set_reaction(c.sigma)
    ip = pm.Interpolator(pc, pf, lc.dofmap, c.lv.dofmap, c.lv.lcells, c.lv.bcells, Lc, c.layout, fine_operator=c.op)
    A = c.oracle(sigma=c.sigma)
    oi = po.Interpolator(pc, pf, lc.dofmap, c.lv.dofmap, lc.ndofs, c.lv.ndofs)
    rng = np.random.default_rng(70 + pf)
    # (r small beside A z, so that the term's share of a restricted boundary row is its share of the apply's)
    zu, ru = rng.standard_normal(c.lv.ndofs), 1e-3 * rng.standard_normal(c.lv.ndofs)
    z, r, coarse = _vec(pm, c.layout, zu), _vec(pm, c.layout, ru), pm.Vector(Lc)
    coarse.set(3.0)
    ip.restrict_residual(c.op, z, r, coarse)
    got = coarse.data_copy()
    ref = oi.reverse_interpolate(ru - A.apply(zu))  # the explicitly formed r - (A + D) z
    without = oi.reverse_interpolate(ru - (A.apply(zu) - A.d_R * zu))
    # the coarse rows the term reaches: those a fine boundary row restricts to
    reach = oi.reverse_interpolate(c.on_facets().astype(np.float64)) > 0
    print(f"{pf} -> {pc}: fused restriction {_relerr(got, ref):.3e}; without d_R "
          f"{_relerr(without[reach], ref[reach]):.3e} away")
    assert _relerr(got, ref) < 1e-12
    assert _relerr(without[reach], ref[reach]) > 1e-2


# ---- 8. inverse diagonal, assembled matrix, AMG level 0 ---------------------------------------------------------------


def test_diagonal_matrix_and_amg_carry_the_term(pm):
    P, n = 1, (4, 4, 4)
    c = Case(pm, n, P, "twist", 80)
    c.op.compute_diag_inverse()
    d_plain = c.diag()
    c.set()
    A = c.oracle()
    mask = c.on_facets()
    # the computed inverse diagonal followed, and the difference of the two is d_R
    assert _relerr(c.diag(), A.diag_inverse()) < 1e-12
    assert _relerr((1.0 / c.diag() - 1.0 / d_plain)[mask], A.d_R[mask]) < 1e-12
    # assembled matrix: the values it was assembled with, then update_values
    M = pm.MatrixOperator(c.op)
    ref = A.dense()
    assert np.abs(M.to_scipy().toarray() - ref).max() < 1e-13 * np.abs(ref).max()
    alpha2 = rb.random_alpha(c.cells.size, (P + 1) ** 2, 81)
    c.set(alpha=alpha2)
    assert np.abs(M.to_scipy().toarray() - ref).max() < 1e-13 * np.abs(ref).max()
    M.update_values()
    A2 = c.oracle(alpha=alpha2)
    ref2 = A2.dense()
    assert np.abs(M.to_scipy().toarray() - ref2).max() < 1e-13 * np.abs(ref2).max()
    assert np.abs(np.diag(ref2 - ref))[mask].max() > 1e-2 * np.abs(np.diag(ref))[mask].max()
    u = np.random.default_rng(82).standard_normal(c.lv.ndofs)
    ym = pm.Vector(c.layout)
    M(_vec(pm, c.layout, u), ym)
    assert _rows(ym.data_copy(), A2.apply(u), u, c.bc) < 1e-12
    assert c.away(A2, u) > 1e-2
    dm = pm.Vector(c.layout)
    M.get_diag_inverse(dm)
    assert _relerr(dm.data_copy(), A2.diag_inverse()) < 1e-12
    # AMG: d_R on the diagonal of level 0
    amg = pm.AmgSolver(c.op, max_iter=60, rtol=1e-9)
    d0 = amg.export(0, "A").diagonal()
    want = A2.diagonal()
    free = ~c.bc.astype(bool)
    assert np.abs(d0 - want)[free].max() < 1e-13 * np.abs(want[free]).max()
    assert np.abs(d0 - A2.A.diagonal())[mask].max() > 1e-2 * np.abs(want[mask]).max()
    c.op.set_robin(None, None, None)  # ... and a removal
    M.update_values()
    plain = A2.A.assemble_csr().toarray()
    assert np.abs(M.to_scipy().toarray() - plain).max() < 1e-13 * np.abs(plain).max()


# ---- 9. V-cycle -------------------------------------------------------------------------------------------------------


def _hierarchy_alpha(seed):
    return lambda pts: rb.random_alpha(len(pts), 1, seed).ravel()


def _oracle_levels(pm, n, orders, kappa, wf, alpha_of, sigma=None, dirichlet=_x0_face):
    part = pm.BoxPartition(n, warp=wf)
    cells, facets = part.exterior_facets()
    ops = []
    for P in orders:
        lv = part.level(P)
        bc = (lv.bc_marker.astype(bool) & dirichlet(part.dof_coordinates(P))).astype(np.int8)
        alpha = alpha_of(part.facet_point_coordinates(P, cells, facets).reshape(-1, 3)).reshape(cells.size, -1)
        ops.append(rb.laplacian(part, P, kappa, lv.dofmap, bc, cells, facets, alpha, sigma))
    return part, ops


def _oracle_cycle(ops, orders, eig_ranges, cheb_its, b, coarse=None):
    from oracle import pmg_oracle as po

    sm = [po.Chebyshev(e, cheb_its) for e in eig_ranges]  # the device run's bounds: the cycle's arithmetic is compared
    it = [po.Interpolator(orders[i], orders[i + 1], ops[i].dofmap, ops[i + 1].dofmap, ops[i].ndofs, ops[i + 1].ndofs)
          for i in range(len(orders) - 1)]
    mg = po.MultigridPreconditioner(ops, sm, it, ops[0].bc, coarse_solver=coarse)
    return mg.apply(b, np.zeros_like(b)), mg


def _cycle(h):
    v = h.new_vector()
    v.set(0.0)
    h.mg.apply(h.rhs[-1], v)
    return v.data_copy()


@pytest.fixture(scope="module")
def vcycle_cases(pm):
    """(hierarchy, oracle operators, oracle cycle) per orders, built once and left unchanged."""
    cache = {}

    def get(orders):
        if orders not in cache:
            n = 4 if orders == (1, 2, 4) else (2, 4, 4)
            h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=bd.warp, robin=_hierarchy_alpha(90),
                                    dirichlet=_x0_face)
            _, ops = _oracle_levels(pm, n, orders, 0.05, bd.warp, _hierarchy_alpha(90))
            ref, _ = _oracle_cycle(ops, orders, h.eig_ranges, 3, h.rhs[-1].data_copy())
            plain = [rb.RobinLaplacian(A.A, np.zeros(A.ndofs)) for A in ops]
            ref0, _ = _oracle_cycle(plain, orders, h.eig_ranges, 3, h.rhs[-1].data_copy())
            cache[orders] = (h, ops, ref, ref0)
        return cache[orders]

    return get


@pytest.mark.parametrize("orders", [(1, 2, 4), (1, 3, 6)], ids=["4-2-1", "6-3-1"])
def test_vcycle_against_the_oracle(pm, vcycle_cases, orders):
    h, ops, ref, ref0 = vcycle_cases(orders)
    assert all(op.has_robin() and not op.has_reaction() for op in h.operators)
    for lv in h.levels:
        assert 0 < lv.bc_marker.sum() < lv.ndofs
    free = ~h.levels[-1].bc_marker.astype(bool)
    h.mg.set_precision("fp64")
    h.mg.set_graph(False)
    eager = _cycle(h)
    e64 = _relerr(eager[free], ref[free])
    away = _relerr(ref0[free], ref[free])
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    _cycle(h)
    replay = _cycle(h)
    assert h.mg.graph_replays() > n0
    g64 = _relerr(replay, eager)
    h.mg.set_graph(False)
    h.mg.set_precision("fp32")
    eager32 = _cycle(h)
    e32 = _relerr(eager32[free], ref[free])
    h.mg.set_graph(True)
    n1 = h.mg.graph_replays()
    _cycle(h)
    replay32 = _cycle(h)
    assert h.mg.graph_replays() > n1
    g32 = _relerr(replay32, eager32)
    h.mg.set_graph(False)
    h.mg.set_precision("fp64")
    print(f"{orders}: FP64 cycle {e64:.3e} (replay vs eager {g64:.3e}), FP32 cycle {e32:.3e} (replay vs eager "
          f"{g32:.3e}); the cycle without d_R is {away:.3e} away")
    assert e64 < 1e-10 and g64 < NOISE * 100  # (replay: the same kernels, sums in any order -- the suite's 1e-12)
    assert e32 < 1e-4 and g32 < 1e-6
    assert away > 1e-2


def test_chebyshev_solve(pm):
    from oracle import pmg_oracle as po

    P, n = 4, (4, 4, 8)
    c = Case(pm, n, P, "twist", 95)
    c.set()
    c.op.compute_diag_inverse()
    A = c.oracle()
    rng_e, _ = po.estimate_eig_range(A, A.ndofs)
    sm = pm.Chebyshev(c.layout, rng_e)
    sm.set_max_iterations(3)
    b = np.random.default_rng(95).standard_normal(c.lv.ndofs)
    x = pm.Vector(c.layout)
    x.set(0.0)
    sm.solve(c.op, x, _vec(pm, c.layout, b))
    ref = po.Chebyshev(rng_e, 3).solve(A, np.zeros_like(b), b)
    ref0 = po.Chebyshev(rng_e, 3).solve(rb.RobinLaplacian(A.A, np.zeros(A.ndofs)), np.zeros_like(b), b)
    mask = c.on_facets()
    assert _relerr(x.data_copy(), ref) < 1e-10
    assert _relerr(ref0[mask], ref[mask]) > 1e-2


# ---- 10. the address rule: a replayed graph sees a second set, and a second component --------------------------------


def test_graph_replay_follows_a_second_set_and_a_second_component(pm):
    n, orders = 4, (1, 2, 4)
    h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=bd.warp, robin=_hierarchy_alpha(100),
                            dirichlet=_x0_face)
    h.mg.set_graph(True)
    b = h.rhs[-1].data_copy()
    _, ops = _oracle_levels(pm, n, orders, 0.05, bd.warp, _hierarchy_alpha(100))
    ref1, _ = _oracle_cycle(ops, orders, h.eig_ranges, 3, b)
    _cycle(h)
    first = _cycle(h)
    n0 = h.mg.graph_replays()
    assert n0 > 0 and _relerr(first, ref1) < 1e-10
    # a second set with other values: the vector is rewritten where the graph reads it
    part, ops2 = _oracle_levels(pm, n, orders, 0.05, bd.warp, _hierarchy_alpha(101))
    cells, facets = part.exterior_facets()
    for P, op in zip(orders, h.operators):
        pts = part.facet_point_coordinates(P, cells, facets).reshape(-1, 3)
        op.set_robin(cells, facets, _hierarchy_alpha(101)(pts).reshape(cells.size, -1))
    second = _cycle(h)
    n1 = h.mg.graph_replays()
    ref2, _ = _oracle_cycle(ops2, orders, h.eig_ranges, 3, b)
    assert n1 > n0  # replayed, not run eagerly
    assert _relerr(second, ref2) < 1e-10
    assert _relerr(ref1, ref2) > 1e-3  # the second operator is another one
    # sigma beside it: the same allocation holds d_sigma + d_R
    sigma = rr.random_sigma(part.ncells, 102)
    for op in h.operators:
        op.set_reaction(sigma)
    third = _cycle(h)
    _, ops3 = _oracle_levels(pm, n, orders, 0.05, bd.warp, _hierarchy_alpha(101), sigma=sigma)
    ref3, _ = _oracle_cycle(ops3, orders, h.eig_ranges, 3, b)
    n2 = h.mg.graph_replays()
    assert n2 > n1
    assert _relerr(third, ref3) < 1e-10
    assert _relerr(ref2, ref3) > 1e-3
    # ... and its removal leaves d_R there
    for op in h.operators:
        op.set_reaction(None)
    assert _relerr(_cycle(h), ref2) < 1e-10
    assert h.mg.graph_replays() > n2


# ---- 11. the manufactured problem with no Dirichlet dof ---------------------------------------------------------------


@pytest.mark.parametrize("P,orders,n", [(2, (1, 2), (3, 3, 3)), (3, (1, 3), (2, 3, 2)), (4, (1, 2, 4), (2, 2, 2))])
def test_problem_without_a_dirichlet_dof(pm, P, orders, n):
    """The unit box, kappa = 2, alpha = (1.1, 0.7, 1.9, 0, 3.1, 0.4) on the six faces, no marked dof on any level; the
    load is the volume term plus g = kappa grad u . n + alpha u through assemble_neumann.  PCG at rtol 1e-12 with the
    V-cycle over the AMG coarse solve returns u at the nodes; the bound is the error of the oracle's Jacobi-CG on the
    same system at the same tolerance plus the suite's 1e-10.
    Measured on an MI355X, library (PCG iterations) / oracle's Jacobi-CG (iterations): P = 2 6.890e-14 (9) /
    1.437e-13 (72), P = 3 2.002e-13 (12) / 1.647e-13 (97), P = 4 1.102e-13 (9) / 1.607e-13 (114)."""
    from oracle import pmg_oracle as po

    part = pm.BoxPartition(n)
    cells, facets = part.exterior_facets()
    face_alpha = np.asarray(rb.FACE_ALPHA_NO_DIRICHLET)

    def robin(pts):  # evaluated on part.exterior_facets(), facet by facet: one constant per box face
        return np.repeat(face_alpha[facets.astype(int)], len(pts) // facets.size)

    h = pm.PoissonHierarchy(n, orders, kappa=bd.KAPPA, cheb_its=3, robin=robin, dirichlet=lambda c: c[:, 0] < -1.0)
    assert all(lv.bc_marker.sum() == 0 for lv in h.levels) and all(op.has_robin() for op in h.operators)
    h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], cycles=2))
    lv, layout, op = h.levels[-1], h.layouts[-1], h.operators[-1]
    u, b_ref, d_R, marker, K = rb.manufactured_problem(part, P, rb.FACE_ALPHA_NO_DIRICHLET, False)
    # the right-hand side through the library: assemble_rhs takes f / kappa, assemble_neumann takes g
    coords = part.dof_coordinates(P)
    uf, gr, lap = bd.exact(P)
    _, normal = bd.facet_geometry(part, P, cells, facets)
    pts = part.facet_point_coordinates(P, cells, facets)
    alpha = np.repeat(face_alpha[facets.astype(int)][:, None], (P + 1) ** 2, axis=1)
    g = (bd.KAPPA * np.einsum("fsd,fsd->fs", gr(pts.reshape(-1, 3)).reshape(pts.shape), normal)
         + alpha * uf(pts.reshape(-1, 3)).reshape(alpha.shape))
    b = pm.Vector(layout)
    op.assemble_rhs(_vec(pm, layout, -lap(coords)), b)
    op.assemble_neumann(cells, facets, g, b)
    assert _relerr(b.data_copy(), b_ref) < 1e-12
    cg = pm.CGSolver(layout)
    cg.set_max_iterations(200)
    cg.set_tolerance(1e-12)
    x = pm.Vector(layout)
    x.set(0.0)
    its = cg.solve(op, x, b, preconditioner=h.mg)
    err = _relerr(x.data_copy(), u)
    A = rb.RobinLaplacian(po.Laplacian(P, bd.KAPPA, lv.dofmap, part.xgeom, part.geom_dofmap, marker), d_R)
    ocg = po.CGSolver()
    ocg.set_max_iterations(5000)
    ocg.set_tolerance(1e-12)
    xo = np.zeros(lv.ndofs)
    oits = ocg.solve(A, xo, b_ref)
    oerr = _relerr(xo, u)
    print(f"no Dirichlet dof, P = {P}: PCG {its} iterations, max|x - u| / max|u| = {err:.3e}; oracle's Jacobi-CG "
          f"{oits} iterations, {oerr:.3e}")
    assert its < 60
    assert err <= oerr + 1e-10


# ---- 12. refusals -----------------------------------------------------------------------------------------------------


def test_refusals_change_nothing(pm):
    from pmg_dolfinx_amd import _lib
    from pmg_dolfinx_amd._lib import current_stream, ptr

    P = 2
    nf = (P + 1) ** 2
    part = pm.BoxPartition((3, 2, 2), warp=bd.twist)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    bc = rb.one_face_marker(lv.bc_marker, part.dof_coordinates(P))
    listed = np.arange(11, dtype=np.int32)  # cell 11 is in neither cell list: the operator does not know it
    kappa = _kappa(P, part.ncells, 110)
    ip, bp = _lib.c_ip, _lib.c_bp
    u = np.random.default_rng(110).standard_normal(lv.ndofs)
    cells, facets = np.array([1, 3, 5, 7], dtype=np.int32), np.array([2, 3, 4, 5], dtype=np.int8)
    good = rb.random_alpha(4, nf, 111)
    for with_term in (False, True):
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, listed,
                                 np.zeros(0, dtype=np.int32), bc, layout)
        if with_term:
            op.set_robin(cells, facets, good)
        op.compute_diag_inverse()
        H, s = op.handle, current_stream()

        def state():
            x, y, d = _vec(pm, layout, u), pm.Vector(layout), pm.Vector(layout)
            y.set(7.0)
            op(x, y)
            op.get_diag_inverse(d)
            torch.cuda.synchronize()
            return y.data.clone(), d.data.clone()

        y0, d0 = state()  # (the inverse diagonal is not recomputed by a refused call: bit for bit; the apply: NOISE)

        def unchanged():
            y, d = state()
            assert op.has_robin() == with_term
            assert torch.equal(d, d0)
            assert _relerr(y.cpu().numpy(), y0.cpu().numpy()) < NOISE

        def refused(c, f, a, count=None, match=b"pmg_laplacian_set_robin"):
            rc = _lib.lib().pmg_laplacian_set_robin(
                H, len(c) if count is None else count, c.ctypes.data_as(ip) if c is not None else None,
                f.ctypes.data_as(bp) if f is not None else None, ptr(a) if a is not None else None, s)
            msg = _lib.lib().pmg_last_error()
            assert rc == -1, rc  # PMG_ERR_INVALID
            assert b"pmg_laplacian_set_robin" in msg and match in msg, msg
            unchanged()

        dev = torch.from_numpy(good).cuda()
        for i, value in enumerate((float("nan"), -1e-300, -2.0, float("inf"))):
            bad = good.copy()
            bad.ravel()[(7 * i + 3) % bad.size] = value
            refused(cells, facets, torch.from_numpy(bad).cuda(), match=b"1 facet points have a value that is not finite")
            with pytest.raises(pm._lib.PmgError, match="1 facet points") as e:
                op.set_robin(cells, facets, bad)
            assert "(code -1)" in str(e.value)
        bad = good.copy()
        bad[1, :3] = -1.0
        bad[2, 0] = float("nan")
        refused(cells, facets, torch.from_numpy(bad).cuda(), match=b"4 facet points")
        for wrong in (-1, part.ncells, 11):  # outside [0, ncells) twice, then a cell the operator does not list
            c = cells.copy()
            c[2] = wrong
            refused(c, facets, dev, match=b"facet 2")
        for wrong in (-1, 6):
            f = facets.copy()
            f[3] = wrong
            refused(cells, f, dev, match=b"outside 0..5")
        refused(None, facets, dev, count=4, match=b"NULL")
        refused(cells, None, dev, count=4, match=b"NULL")
        refused(cells, facets, None, match=b"NULL")
        refused(cells, facets, dev, count=-1, match=b"negative")
        # shape and dtype, from Python
        with pytest.raises(ValueError, match="entries"):
            op.set_robin(cells, facets, good[:-1])
        with pytest.raises(ValueError, match="one length"):
            op.set_robin(cells, facets[:-1], good)
        with pytest.raises(TypeError):
            op.set_robin(cells, facets, dev.float())
        unchanged()
        # inside a stream capture (the pattern of tests/test_gpu_reaction.py: the capture holds one kernel of its own
        # and the refused calls, and is thrown away)
        side, scratch = torch.cuda.Stream(), torch.zeros(8, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                scratch.add_(1.0)
                rc = _lib.lib().pmg_laplacian_set_robin(H, 4, cells.ctypes.data_as(ip), facets.ctypes.data_as(bp),
                                                        ptr(dev), current_stream())
                msg = _lib.lib().pmg_last_error()
                rc0 = _lib.lib().pmg_laplacian_set_robin(H, 0, None, None, None, current_stream())
                msg0 = _lib.lib().pmg_last_error()
        torch.cuda.current_stream().wait_stream(side)
        assert rc == -1 and b"pmg_laplacian_set_robin" in msg and b"stream capture" in msg
        assert rc0 == -1 and b"stream capture" in msg0
        torch.cuda.synchronize()
        unchanged()
        # ... and the call works afterwards
        op.set_robin(cells, facets, dev)
        assert op.has_robin()


# ---- 13. two ranks on one GPU -----------------------------------------------------------------------------------------


def _rank_alpha(pts):
    return 2.0 + np.sin(1.0 + 2 * pts[:, 0] + 3 * pts[:, 1] * pts[:, 2])  # a function of the point: the same on any rank


def _rank_body(rank, world, port, n, dims, degrees):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm

        torch.cuda.set_device(0)
        out = {}
        for P in degrees:
            kap = 0.5 / P**2
            H = pm.PoissonHierarchy(n, (P,), kappa=kap, proc_dims=dims, rank=rank, size=world, warp=bd.warp,
                                    dirichlet=_x0_face)
            lv, layout, op, part = H.levels[0], H.layouts[0], H.operators[0], H.part
            # the single-domain truth, by global dof number
            gp = pm.BoxPartition(n, warp=bd.warp)
            glv = gp.level(P)
            gbc = rb.one_face_marker(glv.bc_marker, gp.dof_coordinates(P))
            gcells, gfacets = gp.exterior_facets()
            galpha = _rank_alpha(gp.facet_point_coordinates(P, gcells, gfacets).reshape(-1, 3)).reshape(gcells.size, -1)
            A = rb.laplacian(gp, P, kap, glv.dofmap, gbc, gcells, gfacets, galpha)
            # each rank lists all exterior facets it holds, ghost cells included
            cells, facets = part.exterior_facets()
            alpha = _rank_alpha(part.facet_point_coordinates(P, cells, facets).reshape(-1, 3)).reshape(cells.size, -1)
            # one rank hands in a bad value: both refuse, nothing changes
            bad = alpha.copy()
            if rank == 1:
                bad[0, 0] = -1.0
            refused = False
            try:
                op.set_robin(cells, facets, bad)
            except pm._lib.PmgError as e:
                refused = "(code -1)" in str(e) and "1 facet points" in str(e)
            still_plain = not op.has_robin()
            op.set_robin(cells, facets, alpha)  # the hierarchy computed the diagonal: it follows
            own = lv.local_to_global[: lv.size_local]
            ug = np.random.default_rng(11).standard_normal(A.ndofs)
            xl = np.zeros(lv.ndofs)
            xl[: lv.size_local] = ug[own]
            x, y, d = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
            x.data.copy_(torch.from_numpy(xl))
            op(x, y)
            op.get_diag_inverse(d)
            ref, dref = A.apply(ug)[own], A.diag_inverse()[own]
            without = (A.apply(ug) - A.d_R * ug)[own]
            free = ~gbc.astype(bool)[own]
            on = np.zeros(glv.ndofs, dtype=bool)
            on[bd.facet_dofs(P, glv.dofmap, gcells, gfacets).ravel()] = True
            mask = (on & ~gbc.astype(bool))[own]
            got = y.data_copy()[: lv.size_local]
            dist.barrier()
            out[P] = {"ghost_cells": int(part.ncells - part.ncells_owned),
                      "ghost_cells_listed": bool((cells >= part.ncells_owned).any()), "refused": refused,
                      "still_plain": still_plain, "has_robin": bool(op.has_robin()),
                      "marked_exact": bool(np.array_equal(got[~free], ug[own][~free])),
                      "apply": float(np.abs(got - ref)[free].max() / np.abs(ref[free]).max()),
                      "away": float(np.abs(without - ref)[mask].max() / np.abs(ref[mask]).max()),
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
    from test_gpu_coefficient_field import _run_ranks  # the suite's launcher: time limits, first failure ends the run

    res = _run_ranks(_rank_worker, 2, ((3, 4, 8), (1, 1, 2), (2, 4)))
    for per_rank in res:
        for P, out in per_rank.items():
            print(P, out)
            assert out["ghost_cells"] > 0 and out["ghost_cells_listed"]
            assert out["refused"] and out["still_plain"] and out["has_robin"], (P, out)
            assert out["marked_exact"], (P, out)
            assert out["apply"] < 1e-12 and out["diag"] < 1e-12, (P, out)
            assert out["away"] > 1e-2, (P, out)
