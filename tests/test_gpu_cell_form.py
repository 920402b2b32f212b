"""The per-cell bilinear form on the device (pmg_laplacian_cell_form, MatFreeLaplacian.cell_form).

Meshes: jittered boxes of 3x2x2 = 12 cells and 5x1x1 = 5 cells and a single cell, so that the last workgroup is partial
at degree 1 (8 cells per workgroup) and at degree 2 (3 cells per workgroup); Dirichlet on the face x = 0 only, so marked
and unmarked dofs share cells; kappa random in [1, 2] per cell.

Bar: every comparison is within 1e-12 * S_c, S_c = sum_q |term_q| of the cell from tests/cell_form_reference.py (the
numpy form written from the weak form, pinned in tests/test_cell_form_abi.py) -- the project's bar for the apply
(tests/test_gpu_parity.py), on the form's own scale.  Statements about bytes use torch.equal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cell_form_reference as cf  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAR = 1e-12
MESHES = {"box12": (3, 2, 2), "row5": (5, 1, 1), "one": (1, 1, 1)}
KAPPA, CONSTRAINED = 1, 2


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def smooth(x):
    """A gentle bend for the degree-2 coordinate element (mid-edge nodes stay well inside their cells)."""
    return x + 0.02 * np.sin(3.0 * x[:, [1, 2, 0]] + 1.0) * np.cos(2.0 * x[:, [2, 0, 1]])


class Case:
    """One operator on one mesh with its host data: everything the reference needs."""

    def __init__(self, pm, n, P, warp=cf.jitter, g=1, seed=0, proc_dims=(1, 1, 1), rank=0):
        self.pm, self.P, self.g = pm, P, g
        self.part = part = pm.BoxPartition(n, proc_dims, rank, warp=warp, geom_degree=g)
        self.lv = lv = part.level(P)
        # the face x = 0 of the unwarped box (the global dof index along x is 0)
        gx = lv.local_to_global // ((n[1] * P + 1) * (n[2] * P + 1))
        self.marker = ((gx == 0) & (lv.bc_marker != 0)).astype(np.int8)
        assert 0 < self.marker.sum() < lv.ndofs
        self.layout = pm.make_layout(lv)
        rng = np.random.default_rng(1000 * P + 10 * part.ncells + seed)
        self.kappa_h = rng.uniform(1.0, 2.0, part.ncells)
        self.kappa = torch.from_numpy(self.kappa_h.copy()).cuda()
        self.op = pm.MatFreeLaplacian(P, self.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                      self.marker, self.layout, geometry_degree=g)
        self.u_h, self.v_h = rng.standard_normal(lv.ndofs), rng.standard_normal(lv.ndofs)
        self.u, self.v = self.dev(self.u_h), self.dev(self.v_h)
        self.kq = self.T = None
        self.rng = rng

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    def vec(self, a):
        x = self.pm.Vector(self.layout)
        x.data.copy_(self.dev(a))
        return x

    def set_field(self):
        self.kq = self.rng.uniform(0.5, 2.0, self.lv.ndofs)
        self.op.set_coefficient_field(self.vec(self.kq))

    def set_tensor(self):
        self.T = tr.random_spd(self.part.ncells, 7)
        self.op.set_coefficient_tensor(self.T)

    def reference(self, flags, u=None, v=None):
        return cf.cell_form(self.P, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap,
                            self.u_h if u is None else u, self.v_h if v is None else v, g=self.g,
                            kappa=self.kappa_h if flags & KAPPA else None,
                            marker=self.marker if flags & CONSTRAINED else None, kq=self.kq, T=self.T)

    def form(self, flags, u=None, v=None):
        return self.op.cell_form(self.u if u is None else u, self.v if v is None else v, kappa=bool(flags & KAPPA),
                                 constrained=bool(flags & CONSTRAINED))

    def check(self, flags, what=""):
        e, S = self.reference(flags)
        got = self.form(flags).cpu().numpy()
        assert got.shape == e.shape
        worst = (np.abs(got - e) / S).max()
        print(f"{what} P={self.P} flags={flags}: max |got - ref| / S_c = {worst:.3e}")
        assert np.all(np.abs(got - e) <= BAR * S), (what, flags, worst)

    def apply(self, x_h):
        x, y = self.vec(x_h), self.pm.Vector(self.layout)
        self.op(x, y)
        return y.data_copy()


def _meshes_for(P):
    # degree 1 and 2: the partial last workgroup (12 = 8 + 4 and 5 cells; 5 = 3 + 2); a single cell at every degree
    return ("box12", "row5", "one") if P <= 2 else (("box12", "one") if P <= 5 else ("row5", "one"))


# ---- 1. against the reference module ------------------------------------------------------------------------------


@pytest.mark.parametrize("P", range(1, 9))
def test_against_the_reference(pm, P):
    for name in _meshes_for(P):
        case = Case(pm, MESHES[name], P)
        for flags in (0, KAPPA, CONSTRAINED, KAPPA | CONSTRAINED):
            case.check(flags, name)


# ---- 2. the sum identity, through the existing apply ------------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 2, 3, 4, 6, 8])
def test_sum_is_the_energy_product_of_the_apply(pm, P):
    case = Case(pm, MESHES["box12" if P <= 4 else "row5"], P, seed=1)
    m = case.marker.astype(bool)
    um, vm = np.where(m, 0.0, case.u_h), np.where(m, 0.0, case.v_h)
    want = vm @ case.apply(um)
    got = case.form(KAPPA | CONSTRAINED).cpu().numpy().sum()
    _, S = case.reference(KAPPA | CONSTRAINED)
    print(f"P={P}: |sum_c e_c - v_m . A u_m| / sum_c S_c = {abs(got - want) / S.sum():.3e}")
    assert abs(got - want) <= BAR * S.sum()


# ---- 3. the exact derivative, through the existing apply ------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 2, 4, 7])
def test_is_the_derivative_of_the_apply_in_kappa(pm, P):
    name = "box12" if P <= 4 else "row5"
    case = Case(pm, MESHES[name], P, seed=2)
    m = case.marker.astype(bool)
    vm = np.where(m, 0.0, case.v_h)
    e = case.form(CONSTRAINED).cpu().numpy()
    y0 = case.apply(case.u_h)
    delta = 0.75
    for c in ((0, 5, 11) if name == "box12" else (0, 2, 4)):
        case.kappa[c] += delta  # in place on the device: the operator reads the caller's array
        y1 = case.apply(case.u_h)
        case.kappa[c] -= delta
        got = vm @ (y1 - y0) / delta
        bar = BAR * (np.abs(vm) @ np.abs(y0) + np.abs(vm) @ np.abs(y1)) / delta
        print(f"P={P} cell {c}: |difference quotient - e_c| / bar = {abs(got - e[c]) / bar:.3e}")
        assert abs(got - e[c]) <= bar


# ---- 4. algebra -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 4])
def test_algebra(pm, P):
    case = Case(pm, MESHES["box12"], P, seed=3)
    for flags in (0, KAPPA | CONSTRAINED):
        _, S = case.reference(flags)
        uv = case.form(flags)
        vu = case.form(flags, u=case.v, v=case.u)
        assert np.all(np.abs((uv - vu).cpu().numpy()) <= BAR * S)  # symmetric
        assert torch.equal(uv, case.form(flags))  # two calls, the same bytes
    uu = case.form(KAPPA, u=case.u, v=case.u)  # one array twice
    assert bool((uu >= 0).all()) and bool((uu > 0).any())
    assert torch.equal(uu, case.form(KAPPA, u=case.u, v=case.u.clone()))  # ... as two copies
    # e_c(1, v) = 0.  The reference's S_c of the pair (1, v) is itself rounding (the constant's gradient is zero), so
    # it is no scale; the bar is the cell's S_c(u, v) with the case's random u, a function of the constant's size
    # (unit variance) on the same cell with the same v: what rounds in the sum D 1 is of the size of the entries of
    # D times the values, as it is for u.
    _, S = case.reference(0)
    e1 = case.form(0, u=case.dev(np.ones(case.lv.ndofs))).cpu().numpy()
    print(f"P={P}: max |e_c(1, v)| / S_c(u, v) = {(np.abs(e1) / S).max():.3e}")
    assert np.all(np.abs(e1) <= BAR * S)


# ---- 5. every state an operator can be in -----------------------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("state", ["field", "tensor", "both", "curved", "batched", "affine", "stream", "recompute",
                                   "diagonal_terms"])
def test_operator_states(pm, P, state):
    n = MESHES["box12"]
    if state == "curved":
        case = Case(pm, n, P, warp=smooth, g=2, seed=4)
    elif state == "affine":
        case = Case(pm, n, P, warp=None, seed=4)
    else:
        case = Case(pm, n, P, seed=4)
    op = case.op
    if state in ("field", "both"):
        case.set_field()
    if state in ("tensor", "both"):
        case.set_tensor()
    if state == "batched":
        pm._lib.call("pmg_laplacian_set_geometry_batch", op.handle, 4)  # > 0: no resident tensor
    if state == "affine":
        assert op.is_affine()
        op.set_geometry_mode("affine")
    if state in ("stream", "recompute"):
        on = state == "recompute"
        if P == 2:
            op.set_tensor_recompute(on)
            assert op.tensor_recomputed() == on
        else:
            if op.chain_form():  # (the degree-4 recomputed form is not for the chain form)
                op.set_chain_form(False)
            op.set_tensor_recompute_identity(on)
            assert op.tensor_recomputed_identity() == on
    if state == "diagonal_terms":
        # the reaction and Robin terms are not part of the form: not a bit moves
        before = [case.form(f).clone() for f in (0, KAPPA | CONSTRAINED)]
        op.set_reaction(case.rng.uniform(0.5, 2.0, case.part.ncells))
        fc, fl = case.part.exterior_facets()
        keep = fl != 0  # (the face x = 0 is Dirichlet)
        op.set_robin(fc[keep], fl[keep], case.rng.uniform(0.5, 2.0, (int(keep.sum()), (P + 1) ** 2)))
        assert op.has_reaction() and op.has_robin()
        for f, b in zip((0, KAPPA | CONSTRAINED), before):
            assert torch.equal(case.form(f), b)
    y = case.apply(case.u_h)  # the state is one the apply runs in
    assert np.isfinite(y).all()
    for flags in (KAPPA, KAPPA | CONSTRAINED):
        case.check(flags, state)


# ---- 6. ghost cells, without communication ---------------------------------------------------------------------------


@pytest.mark.parametrize("rank", [0, 1])
def test_ghost_cells_need_no_exchange(pm, rank):
    P, n = 2, (2, 2, 4)
    whole = Case(pm, n, P, seed=5)
    piece = Case(pm, n, P, seed=5, proc_dims=(1, 1, 2), rank=rank)  # no communicator attached
    assert piece.lv.num_ghosts > 0 and piece.part.ncells > piece.part.ncells_owned
    l2g = piece.lv.local_to_global
    # the global cell behind every local one, ghost cells included (both list cells lexicographically by coordinates)
    cc = piece.part.cell_coords
    gcell = (cc[:, 0] * n[1] + cc[:, 1]) * n[2] + cc[:, 2]
    assert np.array_equal(whole.part.cell_coords[gcell], cc)
    kappa_g = whole.kappa_h
    piece.kappa.copy_(piece.dev(kappa_g[gcell]))
    u, v = piece.dev(whole.u_h[l2g]), piece.dev(whole.v_h[l2g])  # owned and ghost entries, filled on the host
    scatters = piece.layout.forward_scatters()
    for flags in (KAPPA, KAPPA | CONSTRAINED):
        e, S = whole.reference(flags)
        want = whole.form(flags).cpu().numpy()
        got = piece.form(flags, u=u, v=v).cpu().numpy()
        assert got.shape == (piece.part.ncells,)
        assert np.all(np.abs(got - want[gcell]) <= BAR * S[gcell])
        assert np.all(np.abs(got - e[gcell]) <= BAR * S[gcell])
    assert piece.layout.forward_scatters() == scatters


# ---- 7. refusals ------------------------------------------------------------------------------------------------------


def test_refusals_leave_the_output_alone(pm):
    case = Case(pm, MESHES["box12"], 2, seed=6)
    L = pm._lib.lib()
    n = case.lv.ndofs
    buf = torch.full((n + 12,), -7.0, dtype=torch.float64, device="cuda")
    buf[:n] = case.u
    out = torch.full((12,), -7.0, dtype=torch.float64, device="cuda")
    vp, s = pm._lib.vp, pm._lib.current_stream()
    h = case.op.handle

    def refused(u, v, o, flags, word):
        rc = L.pmg_laplacian_cell_form(h, vp(u), vp(v), vp(o) if o else None, flags, s)
        msg = L.pmg_last_error().decode()
        assert rc == -1 and "pmg_laplacian_cell_form" in msg and word in msg, (rc, msg)

    refused(case.u.data_ptr(), case.v.data_ptr(), out.data_ptr(), 4, "flag")
    refused(case.u.data_ptr(), case.v.data_ptr(), out.data_ptr(), KAPPA | 8, "flag")
    refused(case.u.data_ptr(), case.v.data_ptr(), 0, KAPPA, "NULL")
    # out inside u's array: its last entries; and u's array starting inside out
    refused(buf.data_ptr(), case.v.data_ptr(), buf.data_ptr() + 8 * (n - 5), KAPPA, "overlap")
    refused(case.u.data_ptr(), buf.data_ptr(), buf.data_ptr() + 8 * (n - 1), KAPPA, "overlap")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((buf[n:] == -7.0).all()) and torch.equal(buf[:n], case.u)
    # directly behind u: no overlap, accepted
    assert L.pmg_laplacian_cell_form(h, vp(buf.data_ptr()), vp(case.v.data_ptr()), vp(buf.data_ptr() + 8 * n), KAPPA,
                                     s) == 0
    assert torch.equal(buf[n:], case.form(KAPPA))
    # the Python method's own checks
    with pytest.raises(TypeError):
        case.op.cell_form(case.u.float(), case.v)
    with pytest.raises(ValueError):
        case.op.cell_form(case.u[:-1].contiguous(), case.v)
    with pytest.raises(ValueError):
        case.op.cell_form(case.u, case.v, out=torch.empty(11, dtype=torch.float64, device="cuda"))


# ---- 8. capture ---------------------------------------------------------------------------------------------------------


def test_captured_call_replays_the_eager_bytes(pm):
    case = Case(pm, MESHES["box12"], 4, seed=7)
    eager = case.form(KAPPA | CONSTRAINED).clone()
    out = torch.zeros(12, dtype=torch.float64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # one kernel node: a straight line
            case.op.cell_form(case.u, case.v, out=out, kappa=True, constrained=True)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    case.u.mul_(2.0)  # the graph reads the caller's arrays at replay
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, case.form(KAPPA | CONSTRAINED))
