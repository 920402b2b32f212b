"""The coefficient gradients of the form on the device (pmg_laplacian_form_gradients, MatFreeLaplacian.form_gradients).

Meshes: the jittered 3x2x2 box, 12 cells, full workgroups at 3 cells per workgroup (degree 2), and a 7x1x1 row, 7 cells,
a partial last workgroup at 8 (degree 1) and at 3 cells per workgroup; Dirichlet on the face x = 0 only, so marked and
unmarked dofs share cells; kappa random in [1, 2] per cell.

Bar: |got - ref| <= 1e-12 S per cell entry and per dof, S the sum of the magnitudes of the entry's terms from
tests/form_gradients_reference.py (which says what a term is; pinned against the oracle in
tests/test_form_gradients_abi.py) -- the project's bar for the apply on each output's own scale; where S is 0 (a dof no
listed cell touches) the value must be exactly 0.  One departure from "the same sum over |term|" taken point by point:
d_field's terms are the three summands of each point's dot product, kappa_c s pv_d (T_c pu)_d, not the point's total,
because a dof inside a cell gets a single point and the bar would otherwise ask for relative accuracy of a cancelling
dot product; the per-cell outputs keep the point terms.
Difference quotients through the library's own apply carry the bar of tests/test_form_gradients_abi.py.  Statements
about bytes use torch.equal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import form_gradients_reference as fg  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAR = 1e-12
MESHES = {"box12": (3, 2, 2), "row7": (7, 1, 1)}
NAMES = fg.NAMES
ALL = dict(kappa=True, field=True, tensor=True, sigma=True)
CONSTRAINED = 2


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
    """One operator on one mesh with its host data: everything the reference needs.  ``drop``: a cell left out of both
    cell lists."""

    def __init__(self, pm, n, P, warp=fg.jitter, g=1, seed=0, proc_dims=(1, 1, 1), rank=0, drop=None):
        self.pm, self.P, self.g = pm, P, g
        self.part = part = pm.BoxPartition(n, proc_dims, rank, warp=warp, geom_degree=g)
        self.lv = lv = part.level(P)
        gx = lv.local_to_global // ((n[1] * P + 1) * (n[2] * P + 1))
        self.marker = ((gx == 0) & (lv.bc_marker != 0)).astype(np.int8)
        assert 0 < self.marker.sum() < lv.ndofs
        self.layout = pm.make_layout(lv)
        rng = np.random.default_rng(1000 * P + 10 * part.ncells + seed)
        self.kappa_h = rng.uniform(1.0, 2.0, part.ncells)
        self.kappa = torch.from_numpy(self.kappa_h.copy()).cuda()
        lcells, bcells = np.asarray(lv.lcells), np.asarray(lv.bcells)
        self.listed = np.zeros(part.ncells, dtype=bool)
        self.listed[lcells] = True
        self.listed[bcells] = True
        if drop is not None:
            lcells, bcells = lcells[lcells != drop], bcells[bcells != drop]
            self.listed[drop] = False
        self.op = pm.MatFreeLaplacian(P, self.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lcells, bcells,
                                      self.marker, self.layout, geometry_degree=g)
        self.u_h, self.v_h = rng.standard_normal(lv.ndofs), rng.standard_normal(lv.ndofs)
        self.u, self.v = self.dev(self.u_h), self.dev(self.v_h)
        self.kq = self.T = self.sigma = None
        self.rng = rng

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    def vec(self, a):
        x = self.pm.Vector(self.layout)
        x.data.copy_(self.dev(a))
        return x

    def set_field(self, kq=None):
        self.kq = self.rng.uniform(0.5, 2.0, self.lv.ndofs) if kq is None else kq
        self.op.set_coefficient_field(self.vec(self.kq))

    def set_tensor(self, T=None):
        self.T = tr.random_spd(self.part.ncells, 7) if T is None else T
        self.op.set_coefficient_tensor(self.T)

    def set_reaction(self, sigma=None):
        self.sigma = self.rng.uniform(0.0, 3.0, self.part.ncells) if sigma is None else sigma
        self.op.set_reaction(self.sigma)

    def reference(self, constrained, u=None, v=None):
        return fg.form_gradients(self.P, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap,
                                 self.u_h if u is None else u, self.v_h if v is None else v, self.kappa_h, g=self.g,
                                 marker=self.marker if constrained else None, kq=self.kq, T=self.T,
                                 listed=self.listed, ndofs=self.lv.ndofs)

    def grads(self, constrained=True, u=None, v=None, **which):
        return self.op.form_gradients(self.u if u is None else u, self.v if v is None else v,
                                      constrained=constrained, **(which or ALL))

    def check(self, constrained, what="", ref=None):
        ref = self.reference(constrained) if ref is None else ref
        got = self.grads(constrained)
        assert sorted(got) == sorted(NAMES)
        for name in NAMES:
            val, S = ref[name]
            g = got[name].cpu().numpy()
            assert g.shape == val.shape, (name, g.shape, val.shape)
            diff = np.abs(g - val)
            worst = (diff[S > 0] / S[S > 0]).max()
            print(f"{what} P={self.P} constrained={constrained} d_{name}: max |got - ref| / S = {worst:.3e}")
            assert np.all(diff <= BAR * S), (what, name, worst)
        return got

    def apply(self, x_h):
        x, y = self.vec(x_h), self.pm.Vector(self.layout)
        self.op(x, y)
        return y.data_copy()


# ---- 1. against the reference module ------------------------------------------------------------------------------


@pytest.mark.parametrize("P", range(1, 9))
def test_against_the_reference(pm, P):
    # degree 1 and 2: both meshes (full and partial workgroups); above, one cell per workgroup
    for name in (("box12", "row7") if P <= 2 else (("box12",) if P <= 5 else ("row7",))):
        case = Case(pm, MESHES[name], P)
        for constrained in (True, False):
            got = case.check(constrained, name)
        m = case.marker.astype(bool)
        assert bool((got["field"].cpu().numpy()[m] != 0.0).all())  # not zero on marked dofs


# ---- 2. every state an operator can be in -----------------------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("state", ["field", "tensor", "all", "curved", "batched", "affine", "recompute_off"])
def test_operator_states(pm, P, state):
    n = MESHES["box12"]
    if state == "curved":
        case = Case(pm, n, P, warp=smooth, g=2, seed=4)
    elif state == "affine":
        case = Case(pm, n, P, warp=None, seed=4)
    else:
        case = Case(pm, n, P, seed=4)
    op = case.op
    if state in ("field", "all"):
        case.set_field()
    if state in ("tensor", "all"):
        case.set_tensor()
    if state == "all":
        case.set_reaction()
    if state == "batched":
        pm._lib.call("pmg_laplacian_set_geometry_batch", op.handle, 4)  # > 0: no resident tensor
    if state == "affine":
        assert op.is_affine()
        op.set_geometry_mode("affine")
    if state == "recompute_off":
        if P == 2:
            op.set_tensor_recompute(False)
            assert not op.tensor_recomputed()
        else:
            op.set_tensor_recompute_identity(False)
            assert not op.tensor_recomputed_identity()
    y = case.apply(case.u_h)  # the state is one the apply runs in
    assert np.isfinite(y).all()
    for constrained in (True, False):
        case.check(constrained, state)


def test_chain_form(pm, monkeypatch):
    """The chain kernel is degree 4's alone (a degree-2 operator has no chain state), and chains need a row of patches:
    (4, 4, 64) with coloured launches is the smallest mesh on which they exist (tests/test_gpu_reaction.py).  The box is
    not jittered: its cells are 1/64 deep."""
    monkeypatch.setenv("PMG_CHAIN", "2")
    pm.set_merge_threshold(0)
    try:
        case = Case(pm, (4, 4, 64), 4, warp=None, seed=4)
    finally:
        pm.set_merge_threshold(-1)
    assert case.op.chain_available() and case.op.chain_form()
    case.set_tensor()
    assert np.isfinite(case.apply(case.u_h)).all()
    for constrained in (True, False):
        case.check(constrained, "chain")


# ---- 3. the outputs one by one, bytes, guards -------------------------------------------------------------------------


@pytest.mark.parametrize("P,mesh", [(1, "row7"), (2, "row7"), (4, "box12")])
def test_each_output_alone_guards_and_bytes(pm, P, mesh):
    case = Case(pm, MESHES[mesh], P, seed=3)
    case.set_field()
    case.set_tensor()
    nc, n = case.part.ncells, case.lv.ndofs
    sizes = {"kappa": nc, "field": n, "tensor": 6 * nc, "sigma": nc}
    G = 5  # guard elements on both sides of every output
    ref = case.reference(True)
    # one buffer for the four outputs, guards between them; d_field starts as NaN
    buf = torch.full((sum(sizes.values()) + G * 5,), -7.0, dtype=torch.float64, device="cuda")
    views, off = {}, G
    for name in NAMES:
        views[name] = buf[off:off + sizes[name]]
        off += sizes[name] + G
    views["field"].fill_(float("nan"))
    out = {k: (v.view(nc, 6) if k == "tensor" else v) for k, v in views.items()}
    res = case.op.form_gradients(case.u, case.v, out=out, **ALL)
    torch.cuda.synchronize()
    assert all(res[k].data_ptr() == views[k].data_ptr() for k in NAMES)
    assert bool(torch.isfinite(views["field"]).all())
    guard = torch.ones_like(buf, dtype=torch.bool)
    for name in NAMES:
        guard[views[name].data_ptr() // 8 - buf.data_ptr() // 8:][:sizes[name]] = False
        val, S = ref[name]
        assert np.all(np.abs(views[name].cpu().numpy().reshape(val.shape) - val) <= BAR * S), name
    assert int(guard.sum()) == 5 * G and bool((buf[guard] == -7.0).all())
    everything = {k: views[k].clone() for k in NAMES}
    # two calls: the same bytes in the per-cell outputs, d_field to rounding
    again = case.grads(True)
    for name in NAMES:
        if name == "field":
            assert np.all(np.abs((again[name] - everything[name]).cpu().numpy()) <= BAR * ref[name][1])
        else:
            assert torch.equal(again[name].reshape(-1), everything[name])
    # each output alone: the others, and all the guards, untouched; per-cell outputs byte for byte
    for name in NAMES:
        buf.fill_(-7.0)
        res = case.op.form_gradients(case.u, case.v, out={name: out[name]}, **{name: True})
        torch.cuda.synchronize()
        assert list(res) == [name]
        mine = torch.zeros_like(buf, dtype=torch.bool)
        mine[views[name].data_ptr() // 8 - buf.data_ptr() // 8:][:sizes[name]] = True
        assert bool((buf[~mine] == -7.0).all()), name
        if name == "field":
            assert np.all(np.abs((views[name] - everything[name]).cpu().numpy()) <= BAR * ref[name][1])
        else:
            assert torch.equal(views[name], everything[name]), name


@pytest.mark.parametrize("P", [1, 2, 4])
def test_d_kappa_is_the_cell_form(pm, P):
    case = Case(pm, MESHES["row7"], P, seed=8)
    case.set_field()
    case.set_tensor()
    for constrained in (True, False):
        e = case.op.cell_form(case.u, case.v, kappa=False, constrained=constrained).cpu().numpy()
        got = case.grads(constrained, kappa=True)["kappa"].cpu().numpy()
        S = case.reference(constrained)["kappa"][1]
        assert np.all(np.abs(got - e) <= BAR * S)


@pytest.mark.parametrize("P", [1, 2, 3])
def test_unlisted_cell_leaves_its_own_dofs_exactly_zero(pm, P):
    n = MESHES["box12"]
    drop = 11  # the corner cell at the far end: its corner dof, and at P >= 2 its interior, belong to it alone
    case = Case(pm, n, P, seed=9, drop=drop)
    count = np.zeros(case.lv.ndofs, dtype=int)
    dm = np.asarray(case.lv.dofmap).reshape(case.part.ncells, -1)
    np.add.at(count, dm[case.listed].ravel(), 1)
    alone = np.flatnonzero(count == 0)
    assert alone.size >= 1 and set(alone) <= set(dm[drop])
    ref = case.reference(True)
    assert np.all(ref["field"][1][alone] == 0.0) and np.all(ref["field"][1][count > 0] > 0.0)
    out = {"field": torch.full((case.lv.ndofs,), float("nan"), dtype=torch.float64, device="cuda")}
    got = case.op.form_gradients(case.u, case.v, out=out, **ALL)
    f = got["field"].cpu().numpy()
    assert np.all(f[alone] == 0.0) and not np.signbit(f[alone]).any()
    case.check(True, "unlisted", ref)  # the per-cell outputs have a value for the unlisted cell too
    assert ref["kappa"][1][drop] > 0.0


def test_nan_in_marked_entries_stays_out(pm):
    case = Case(pm, MESHES["box12"], 3, seed=10)
    case.set_field()
    ref = case.reference(True)
    m = torch.from_numpy(case.marker.astype(bool)).cuda()
    u, v = case.u.clone(), case.v.clone()
    u[m] = float("nan")
    v[m] = float("nan")
    got = case.grads(True, u=u, v=v)
    for name in NAMES:
        g = got[name].cpu().numpy()
        assert np.isfinite(g).all() and np.all(np.abs(g - ref[name][0]) <= BAR * ref[name][1]), name
    assert not torch.isfinite(case.grads(False, u=u, v=v)["kappa"]).all()  # (without the flag they are read)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------


def test_refusals_leave_the_outputs_alone(pm):
    case = Case(pm, MESHES["box12"], 2, seed=6)
    L = pm._lib.lib()
    n, nc = case.lv.ndofs, case.part.ncells
    buf = torch.full((n + 6 * nc,), -7.0, dtype=torch.float64, device="cuda")
    buf[:n] = case.u
    outs = {k: torch.full((s,), -7.0, dtype=torch.float64, device="cuda")
            for k, s in (("kappa", nc), ("field", n), ("tensor", 6 * nc), ("sigma", nc))}
    vp, s = pm._lib.vp, pm._lib.current_stream()
    h = case.op.handle
    up, vq = case.u.data_ptr(), case.v.data_ptr()
    dk, df, dt, ds = (outs[k].data_ptr() for k in NAMES)

    def refused(hh, u, v, o, flags, word):
        rc = L.pmg_laplacian_form_gradients(hh, vp(u) if u else None, vp(v) if v else None,
                                            *[vp(p) if p else None for p in o], flags, s)
        msg = L.pmg_last_error().decode()
        assert rc == -1 and "pmg_laplacian_form_gradients" in msg and word in msg, (rc, msg)

    refused(None, up, vq, (dk, df, dt, ds), 0, "NULL")
    refused(h, 0, vq, (dk, df, dt, ds), 0, "NULL")
    refused(h, up, 0, (dk, df, dt, ds), 0, "NULL")
    refused(h, up, vq, (0, 0, 0, 0), CONSTRAINED, "outputs")
    refused(h, up, vq, (dk, df, dt, ds), 1, "flag")  # PMG_CELL_FORM_KAPPA
    refused(h, up, vq, (dk, df, dt, ds), CONSTRAINED | 1, "flag")
    refused(h, up, vq, (dk, df, dt, ds), 4, "flag")
    # an output inside u's array; u's array starting inside an output; two outputs sharing memory
    refused(h, buf.data_ptr(), vq, (buf.data_ptr() + 8 * (n - 5), 0, 0, 0), 0, "overlap")
    refused(h, up, buf.data_ptr(), (0, 0, buf.data_ptr() + 8 * (n - 1), 0), 0, "overlap")
    refused(h, up, vq, (0, df, 0, df + 8 * (n - 1)), 0, "overlap")
    refused(h, up, vq, (dk, df, dt, dk), 0, "overlap")
    refused(h, up, vq, (dt + 8 * (6 * nc - 1), 0, dt, 0), 0, "overlap")
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs.values())
    assert bool((buf[n:] == -7.0).all()) and torch.equal(buf[:n], case.u)
    # directly behind u, and the outputs back to back: no overlap, accepted
    assert L.pmg_laplacian_form_gradients(h, vp(buf.data_ptr()), vp(vq), None, None, vp(buf.data_ptr() + 8 * n), None,
                                          0, s) == 0
    assert torch.equal(buf[n:], case.grads(False, u=buf[:n], tensor=True)["tensor"].reshape(-1))
    # the Python method's own checks
    with pytest.raises(TypeError):
        case.op.form_gradients(case.u.float(), case.v, kappa=True)
    with pytest.raises(ValueError):
        case.op.form_gradients(case.u[:-1].contiguous(), case.v, kappa=True)
    with pytest.raises(ValueError):
        case.op.form_gradients(case.u, case.v)
    with pytest.raises(ValueError):
        case.op.form_gradients(case.u, case.v, kappa=True, out={"kappa": outs["field"]})
    with pytest.raises(ValueError):
        case.op.form_gradients(case.u, case.v, kappa=True, out={"sigma": outs["sigma"]})


# ---- 5. the exact derivative and the Euler identities, through the library's own apply --------------------------------


def _spd(T):
    xx, xy, xz, yy, yz, zz = np.asarray(T).T
    det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz)
    return bool(np.all(xx > 0) and np.all(xx * yy - xy * xy > 0) and np.all(det > 0))


@pytest.mark.parametrize("P", [1, 2, 4])
def test_is_the_derivative_of_the_apply_in_every_coefficient(pm, P):
    case = Case(pm, MESHES["box12"], P, seed=2)
    case.set_field()
    case.set_tensor()
    case.set_reaction()
    m = case.marker.astype(bool)
    vm = np.where(m, 0.0, case.v_h)
    got = {k: t.cpu().numpy() for k, t in case.grads(True).items()}
    y0 = case.apply(case.u_h)
    kq0, T0, s0 = case.kq.copy(), case.T.copy(), case.sigma.copy()

    def check(what, want, delta):
        y1 = case.apply(case.u_h)
        dq = vm @ (y1 - y0) / delta
        bar = BAR * (np.abs(vm) @ np.abs(y0) + np.abs(vm) @ np.abs(y1)) / abs(delta)
        print(f"P={P} {what}: |difference quotient - gradient| / bar = {abs(dq - want) / bar:.3e}")
        assert abs(dq - want) <= bar, what

    # the field: a dof inside cell 0 (at P = 1: a vertex inside the box), a dof inside the face between cell 0 and its
    # neighbour (at P = 1: a vertex inside a face of the box), a marked dof
    nd = P + 1
    dm = np.asarray(case.lv.dofmap).reshape(case.part.ncells, -1)
    count = np.bincount(dm.ravel(), minlength=case.lv.ndofs)
    cell0 = dm[0].reshape(nd, nd, nd)
    inner, shared = int(cell0[1, 1, 1]), int(cell0[nd - 1, 1, 1])
    if P == 1:
        shared = int(np.flatnonzero((count == 4) & ~m)[0])
    assert (count[inner], count[shared]) == ((1, 2) if P >= 2 else (8, 4)) and not m[inner] and not m[shared]
    marked = int(np.flatnonzero(m)[3])
    for n in (inner, shared, marked):
        kq1 = kq0.copy()
        kq1[n] += 0.75
        case.set_field(kq1)
        check(f"field[{n}] (shared by {count[n]} cells, marked {bool(m[n])})", got["field"][n], 0.75)
    case.set_field(kq0)
    # the tensor: a step up a diagonal entry keeps the leading minors positive, and so does an off-diagonal step of
    # 0.25 on eigenvalues of at least 0.5
    for c, k, d in ((5, 3, 0.75), (11, 1, 0.25)):
        T1 = T0.copy()
        T1[c, k] += d
        assert _spd(T0) and _spd(T1)
        case.set_tensor(T1)
        check(f"tensor[{c}][{k}]", got["tensor"][c, k], d)
    case.set_tensor(T0)
    s1 = s0.copy()
    s1[7] += 0.75
    case.set_reaction(s1)
    check("sigma[7]", got["sigma"][7], 0.75)


@pytest.mark.parametrize("P", [1, 2, 4, 7])
def test_euler_identities_against_the_apply(pm, P):
    case = Case(pm, MESHES["box12" if P <= 4 else "row7"], P, seed=1)
    case.set_field()
    case.set_tensor()
    m = case.marker.astype(bool)
    um, vm = np.where(m, 0.0, case.u_h), np.where(m, 0.0, case.v_h)
    want = vm @ case.apply(um)  # (no reaction term: A is A_diff)
    got = {k: t.cpu().numpy() for k, t in case.grads(True).items()}
    ref = case.reference(True)
    sums = {"kappa": (case.kappa_h @ got["kappa"], case.kappa_h @ ref["kappa"][1]),
            "field": (case.kq @ got["field"], case.kq @ ref["field"][1]),
            "tensor": ((case.T * got["tensor"]).sum(), (np.abs(case.T) * ref["tensor"][1]).sum())}
    for name, (val, S) in sums.items():
        print(f"P={P} {name}: |sum - v_m . A u_m| / S = {abs(val - want) / S:.3e}")
        assert abs(val - want) <= BAR * S, name
    # the reaction term's: v_m . (A + d) u_m - v_m . A u_m = sum_c sigma_c d_sigma[c]
    case.set_reaction()
    with_d = vm @ case.apply(um)
    S = case.sigma @ ref["sigma"][1] + sums["kappa"][1]
    assert abs((with_d - want) - case.sigma @ got["sigma"]) <= BAR * S


# ---- 6. capture -------------------------------------------------------------------------------------------------------


def test_captured_call_replays_the_eager_result(pm):
    case = Case(pm, MESHES["box12"], 4, seed=7)
    case.set_field()
    eager = {k: t.clone() for k, t in case.grads(True).items()}
    ref = case.reference(True)
    out = {k: torch.zeros_like(t) for k, t in eager.items()}
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # a fill and a kernel: a straight line
            case.op.form_gradients(case.u, case.v, out=out, **ALL)
    torch.cuda.current_stream().wait_stream(side)

    def same(eager):
        for k in NAMES:
            if k == "field":
                assert np.all(np.abs((out[k] - eager[k]).cpu().numpy()) <= BAR * ref[k][1])
            else:
                assert torch.equal(out[k], eager[k]), k

    for t in out.values():
        t.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    same(eager)
    graph.replay()  # d_field is filled with zeros again, not added to
    torch.cuda.synchronize()
    same(eager)


# ---- 7. two ranks' operators on one GPU ---------------------------------------------------------------------------------


@pytest.mark.parametrize("rank", [0, 1])
def test_owned_field_entries_are_complete_on_a_ghost_layer_partition(pm, rank):
    P, n = 2, (2, 2, 4)
    whole = Case(pm, n, P, seed=5)
    piece = Case(pm, n, P, seed=5, proc_dims=(1, 1, 2), rank=rank)  # no communicator attached
    assert piece.lv.num_ghosts > 0 and piece.part.ncells > piece.part.ncells_owned
    l2g = piece.lv.local_to_global
    cc = piece.part.cell_coords
    gcell = (cc[:, 0] * n[1] + cc[:, 1]) * n[2] + cc[:, 2]
    assert np.array_equal(whole.part.cell_coords[gcell], cc)
    piece.kappa.copy_(piece.dev(whole.kappa_h[gcell]))
    # (no nodal field: setting one scatters it to the ghosts, and no communicator is attached)
    T = tr.random_spd(whole.part.ncells, 7)
    whole.T = T  # (the reference's; the single-domain operator itself is not needed)
    piece.set_tensor(T[gcell])
    u, v = piece.dev(whole.u_h[l2g]), piece.dev(whole.v_h[l2g])  # owned and ghost entries, filled on the host
    scatters = piece.layout.forward_scatters()
    # (the marker of the piece is the whole's, restricted)
    assert np.array_equal(piece.marker, whole.marker[l2g])
    ref = whole.reference(True)
    got = {k: t.cpu().numpy() for k, t in piece.grads(True, u=u, v=v).items()}
    assert piece.layout.forward_scatters() == scatters  # no exchange
    owned = slice(0, piece.lv.size_local)
    val, S = ref["field"]
    assert np.all(np.abs(got["field"][owned] - val[l2g][owned]) <= BAR * S[l2g][owned])
    for name in ("kappa", "tensor", "sigma"):  # every cell of the dofmap, ghost cells included
        val, S = ref[name]
        assert np.all(np.abs(got[name] - val[gcell]) <= BAR * S[gcell]), name
    # ghost entries: this rank's cells only
    mine = fg.form_gradients(P, piece.lv.dofmap, piece.part.xgeom, piece.part.geom_dofmap, whole.u_h[l2g], whole.v_h[l2g],
                             whole.kappa_h[gcell], marker=piece.marker, T=T[gcell], listed=piece.listed,
                             ndofs=piece.lv.ndofs)["field"]
    assert np.all(np.abs(got["field"] - mine[0]) <= BAR * mine[1])
