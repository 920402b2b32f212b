"""The column-constant branch of the recomputed tensor (pmg_laplacian_set_column_tensor; TensorStream's
column_constant in pmg-dolfinx_amd/csrc/stiffness_layer.hpp): a work item -- the cells one wavefront marches through
together -- whose Jacobian does not change down its columns forms adj(J) adj(J)^T / |det J| once instead of once per
layer; every other item runs the general march.  Degrees 2 and 4, the column kernels and the fused (2, 1) and (4, 2)
restrictions, switch on and off, against the oracle and against each other.  Degree 1 has the recomputed form without
the branch (column_branch, stiffness_column.hpp: left out by measurement, profiles/column_tensor.md); what is checked
there is that its operator says so and that a hierarchy's degree-1 level does not move with the switch.

Meshes (4 x 4 x 16 cells; all coordinates multiples of 2^-15 below 2, so the coefficient differences are exact and a
vanishing zeta-cross coefficient is an exact zero):
  box       every item qualifies
  extruded  x and y jittered identically on every z level, z levels non-uniform, the extrusion direction sheared:
            constant down a column, not constant in the cell.  Every item qualifies.
  level     the extruded mesh with the vertices of one interior z level jittered individually: two layers of cells
            do not qualify
  vertex    the extruded mesh with ONE vertex jittered: eight cells do not qualify
  jittered  every interior vertex jittered: no cell qualifies
  frames    the extruded mesh with cells in permuted local frames (frames_for of tests/test_gpu_cell_frames.py): where
            the extrusion axis is local xi or eta the cell does not qualify.  (On a plain box every frame qualifies --
            a box cell has no cross coefficient at all -- so the frames are put on the extruded mesh.)
pmg_laplacian_column_tensor_items says which path a mesh exercised; test_an_item_pairs_both_kinds shows that `level`
and `vertex` hold items that pair a qualifying cell with one that is not.

Bounds, those of tests/test_gpu_tensor_recompute_identity.py: 1e-12 of max |y| for one application or transfer, against
the oracle and between the two settings; 1e-10 after V-cycles.  The two settings differ by where w_k multiplies (the
tensor, or the fluxes): same value to rounding."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402
from test_gpu_tensor_recompute import TOL, TOL_CYCLE, _apply, _cycles, _kappa, _operator, _relerr, _vec, pm  # noqa: E402,F401
from test_tensor_recompute_identity import cell_coefficients  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = (4, 4, 16)
CYCLE_N = (8, 8, 16)
COLUMN = (1, 1, 16)
MESHES = ("box", "extruded", "level", "vertex", "jittered", "frames")
DEGREES = (2, 4)  # degrees with the branch (column_branch)
CW = {2: 7, 4: 2}  # cells of a work item (Shape<P>::CW, stiffness_column.hpp)
Q = 2.0 ** -12
OBSERVED = {"settings": 0.0}


def _q(d):
    return np.round(d / Q) * Q


def warp_of(mesh, n, everywhere=False):
    """The vertex map of a mesh, a fixed function of the vertex's place in the unit box (the oracle's mesh and the
    library's are built separately).  everywhere: the jitter moves the box's boundary vertices too (the 1 x 1 x 16
    column has no others)."""
    if mesh == "box":
        return None
    h = 1.0 / np.asarray(n, dtype=np.float64)

    def inside(x, axes):
        return np.all((x[:, axes] > 1e-9) & (x[:, axes] < 1.0 - 1e-9), axis=1)

    def extrude(x):
        y = x.copy()
        xy = inside(x, [0, 1])
        y[:, 0] += _q(0.2 * h[0] * np.sin(37.0 * x[:, 1] + 91.0 * x[:, 0] + 1.0)) * xy
        y[:, 1] += _q(0.2 * h[1] * np.sin(53.0 * x[:, 0] + 71.0 * x[:, 1] + 2.0)) * xy
        y[:, 2] += _q(0.3 * h[2] * np.sin(29.0 * x[:, 2] + 3.0)) * inside(x, [2])
        y[:, 0] += 0.125 * y[:, 2]  # the extrusion direction (0.125, 0, 1)
        return y

    def each(x):
        return _q(0.15 * h * np.sin(37.0 * x[:, [1, 2, 0]] + 91.0 * x + np.array([1.0, 2.0, 3.0])))

    def f(x):
        if mesh == "jittered":
            return x + each(x) * (1.0 if everywhere else inside(x, [0, 1, 2])[:, None])
        y = extrude(x)
        if mesh == "level":
            y += each(x) * np.isclose(x[:, 2], 5.0 / 16.0)[:, None]
        elif mesh == "vertex":
            at = np.array([(n[0] // 2) / n[0], (n[1] // 4) / n[1], 9.0 / 16.0])
            y += each(x) * np.all(np.isclose(x, at), axis=1)[:, None]
        return y

    return f


_PARTS = {}


def _part(pm, mesh, n=N):
    key = (mesh, n)
    if key not in _PARTS:
        frames = None
        if mesh == "frames":
            from test_gpu_cell_frames import frames_for

            frames = frames_for(pm, n, "mixed")
        _PARTS[key] = pm.BoxPartition(n, warp=warp_of("extruded" if mesh == "frames" else mesh, n, n == COLUMN),
                                      cell_frames=frames)
    return _PARTS[key]


def cells_that_qualify(part):
    """Per cell: do c101, c011 and c111 vanish?  From the differences cell_coefficient_kernel forms, on the cell's
    vertices in its own frame."""
    v = part.xgeom[part.geom_dofmap]
    return np.array([not np.any(cell_coefficients(c)[[3, 5, 7]]) for c in v])


def _items(op):
    q, total = op.column_tensor_items()
    assert 0 <= q <= total and total > 0
    return q, total


def check_items(mesh, part, op, P):
    """The getter against what the mesh was built to exercise, and against the cells counted on the host."""
    q, total = _items(op)
    cells = cells_that_qualify(part)
    print(f"items {mesh} P={P}: {q} of {total} qualify; cells {int(cells.sum())} of {cells.size}")
    if mesh in ("box", "extruded"):
        assert cells.all() and q == total
    elif mesh == "jittered":
        assert not cells.any() and q == 0
    elif mesh == "frames":  # (a cell in three qualifies: at degrees 1 and 2 hardly an item of 16 or 7 cells does)
        assert cells.any() and not cells.all() and q < total
    else:
        # (fewer non-qualifying cells than items, so some item holds none of them: strictly between none and all)
        assert cells.any() and not cells.all() and (~cells).sum() < total and 0 < q < total
    assert total * CW[P] >= cells.size
    # (an item holds at least one cell and at most CW; `spare` slots hold none)
    spare = total * CW[P] - cells.size
    assert (total - q) <= (~cells).sum() and q * CW[P] - spare <= cells.sum()
    return q, total, cells


_REFS = {}


def _reference(part, mesh, P, markers, reaction):
    key = (mesh, P, markers, reaction)
    if key not in _REFS:
        lv = part.level(P)
        bc = lv.bc_marker if markers else np.zeros_like(lv.bc_marker)
        sigma = rr.random_sigma(part.ncells, 11) if reaction else np.zeros(part.ncells)
        A = rr.laplacian(P, _kappa(part.ncells), sigma, lv.dofmap, part.xgeom, part.geom_dofmap, bc)
        u = np.random.default_rng(7 + P).standard_normal(lv.ndofs)
        _REFS[key] = (bc, sigma, u, A.apply(u))
    return _REFS[key]


def _recomputes(op):
    return op.tensor_recomputed() or op.tensor_recomputed_identity()


@pytest.mark.parametrize("reaction", [False, True])
@pytest.mark.parametrize("markers", [True, False])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("mesh", MESHES)
def test_apply_both_settings_against_oracle(pm, mesh, P, markers, reaction):
    part = _part(pm, mesh)
    bc, sigma, u, ref = _reference(part, mesh, P, markers, reaction)
    for coloured in (True, False):
        lv, layout, op = _operator(pm, part, P, bc, coloured)  # (a per-cell kappa that varies: _kappa)
        if P == 4:  # (eight patches: a launch per colour, or one for all)
            assert op.launches_per_apply() > 2 if coloured else op.launches_per_apply() <= 2
        assert _recomputes(op) and op.column_tensor()  # the automatic choice: on
        check_items(mesh, part, op, P)
        if reaction:
            op.set_reaction(sigma)
        out = {}
        for on in (False, True):
            op.set_column_tensor(on)
            assert op.column_tensor() == on and _recomputes(op)
            for rep in range(2):  # the second call: another fill of y, no dependence on what the first left behind
                out[on] = _apply(pm, op, layout, u, fill=3.0 + rep)
                err = _relerr(out[on], ref)
                print(f"apply {mesh} P={P} coloured={coloured} column tensor={on} call {rep}: vs oracle {err:.3e}")
                assert err < TOL
                if markers:  # Dirichlet rows: y = x exactly
                    rows = np.nonzero(bc)[0]
                    assert np.array_equal(out[on][rows], u[rows])
        diff = _relerr(out[True], out[False])
        OBSERVED["settings"] = max(OBSERVED["settings"], diff)
        print(f"apply {mesh} P={P} coloured={coloured}: on vs off {diff:.3e} (largest so far {OBSERVED['settings']:.3e})")
        assert diff < TOL
        op.set_column_tensor(None)
        assert op.column_tensor()


@pytest.mark.parametrize("pair", [(1, 2), (2, 4)])
@pytest.mark.parametrize("mesh", MESHES)
def test_fused_restriction_both_settings(pm, mesh, pair):
    from oracle import pmg_oracle as po

    part = _part(pm, mesh)
    pc, pf = pair
    lc = part.level(pc)
    A = po.Laplacian(pf, _kappa(part.ncells), part.level(pf).dofmap, part.xgeom, part.geom_dofmap,
                     part.level(pf).bc_marker)
    oi = po.Interpolator(pc, pf, lc.dofmap, part.level(pf).dofmap, lc.ndofs, part.level(pf).ndofs)
    rng = np.random.default_rng(21)
    zu, ru = rng.standard_normal(part.level(pf).ndofs), rng.standard_normal(part.level(pf).ndofs)
    ref = oi.reverse_interpolate(ru - A.apply(zu))
    for coloured in (True, False):
        Lc = pm.make_layout(lc)
        lf, Lf, fop = _operator(pm, part, pf, part.level(pf).bc_marker, coloured)
        ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
        z, r, coarse = _vec(pm, Lf, zu), _vec(pm, Lf, ru), pm.Vector(Lc)
        out = {}
        for on in (False, True):
            fop.set_column_tensor(on)
            assert fop.column_tensor() == on
            for rep in range(2):
                coarse.set(3.0)
                ip.restrict_residual(fop, z, r, coarse)
                out[on] = coarse.data_copy()
                err = _relerr(out[on], ref)
                print(f"fused {pair} {mesh} coloured={coloured} column tensor={on} call {rep}: vs oracle {err:.3e}")
                assert err < TOL
        diff = _relerr(out[True], out[False])
        print(f"fused {pair} {mesh} coloured={coloured}: on vs off {diff:.3e}")
        assert diff < TOL


def test_an_item_pairs_both_kinds(pm):
    """Between them, `level` and `vertex` hold an item with a qualifying and a non-qualifying cell.  The items that do
    not qualify have (total - q) CW slots, of which at most `spare` = total CW - cells hold no cell; more cells in them
    than there are non-qualifying cells means a qualifying cell sits in one of them."""
    paired = []
    for mesh in ("level", "vertex"):
        part = _part(pm, mesh)
        for P in DEGREES:
            lv, layout, op = _operator(pm, part, P, part.level(P).bc_marker)
            q, total, cells = check_items(mesh, part, op, P)
            spare = total * CW[P] - cells.size
            if (total - q) * CW[P] - spare > (~cells).sum():
                paired.append((mesh, P))
    print(f"items that pair both kinds: {paired}")
    assert paired


def _switch(h, on):
    for op in h.operators:
        if op.degree in DEGREES:
            op.set_column_tensor(on)
    return [op.column_tensor() for op in h.operators]


@pytest.mark.parametrize("mesh", ["box", "extruded", "level"])
def test_cycles_both_settings(pm, mesh):
    from oracle import pmg_oracle as po

    orders = (1, 2, 4)
    warp = warp_of(mesh, CYCLE_N)
    h = pm.PoissonHierarchy(CYCLE_N, orders, kappa=2.0, cheb_its=3, warp=warp)
    _, _, sm, _, mg, b, _ = po.build_hierarchy(CYCLE_N, orders, cheb_its=3, warp=warp)
    for s, e in zip(sm, h.eig_ranges):  # the device's smoother bounds: only the cycle's arithmetic is compared
        s.eig_range = e
    xo, ref = np.zeros_like(b), []
    for _ in range(3):
        xo = mg.apply(b, xo)
        ref.append(xo.copy())
    for op in h.operators[1:]:  # (on `level` the cycle takes both paths at both degrees)
        check_items(mesh, h.part, op, op.degree)
    h.mg.set_graph(False)
    res, counts, fused = {}, {}, {}
    for on in (True, False):
        assert _switch(h, on) == [False, on, on]
        res[on] = _cycles(h)
        counts[on], fused[on] = h.mg.apply_counts(), h.mg.fused_restrictions()
        for c, (got, want) in enumerate(zip(res[on], ref)):
            err = _relerr(got, want)
            print(f"cycle {mesh} column tensor={on}, cycle {c}: rel.err vs oracle {err:.3e}")
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
        for a, b_ in zip(got, res[on]):
            assert _relerr(a, b_) < TOL
    h.mg.set_graph(False)


@pytest.mark.parametrize("P", DEGREES)
def test_general_path_is_the_arithmetic_it_was(pm, P):
    """A 1 x 1 x 16 column with every vertex jittered: every dof has at most two addends (a + b = b + a), so the
    products are reproducible (tests/test_gpu_chebyshev_recompute.py), and no item qualifies, so switch on and switch
    off must agree bit for bit -- the apply, and the fused restriction of the degrees that have one."""
    part = _part(pm, "jittered", COLUMN)
    lv, layout, op = _operator(pm, part, P, part.level(P).bc_marker)
    assert _items(op)[0] == 0 and not cells_that_qualify(part).any()
    u = np.random.default_rng(5).standard_normal(lv.ndofs)
    out = {}
    for on in (False, True, False):
        op.set_column_tensor(on)
        got = _apply(pm, op, layout, u)
        assert on not in out or np.array_equal(out[on], got)  # (the same setting twice: reproducible here)
        out[on] = got
    assert np.array_equal(out[True], out[False])
    pc = P // 2
    lc = part.level(pc)
    Lc = pm.make_layout(lc)
    ip = pm.Interpolator(pc, P, lc.dofmap, lv.dofmap, lv.lcells, lv.bcells, Lc, layout, fine_operator=op)
    z, r, coarse = _vec(pm, layout, u), _vec(pm, layout, u[::-1].copy()), pm.Vector(Lc)
    for on in (False, True):
        op.set_column_tensor(on)
        coarse.set(3.0)
        ip.restrict_residual(op, z, r, coarse)
        out[on] = coarse.data_copy()
    assert np.array_equal(out[True], out[False])
