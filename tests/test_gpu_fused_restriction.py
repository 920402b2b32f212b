"""The restriction fused into the pre-smooth's last operator application (stiffness_restrict_kernel,
pmg_interpolator_restrict_residual, pmg_multigrid_set_fused_restriction): the kernel alone against the numpy oracle
R (r - A z) and against the library's own unfused sequence, the V-cycle with and without it, and the configurations
in which the cycle must run as before.  Tolerances: 1e-12 per apply / transfer (test_apply_parity_*,
test_transfer_parity) and eager against graph, 1e-10 after a V-cycle (test_vcycle_parity)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def warp(x):
    """Curved grid lines, every cell a parallelepiped (tests/test_gpu_parity.py)."""
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    """Genuinely trilinear cells; the patches of this mesh are Morton chunks, not tensor blocks."""
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


SHEAR = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])


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


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


# (coarse degree, fine degree, cells): the smallest meshes that reach every branch of the kernel
SHAPES = [
    (2, 4, (4, 4, 16)),  # eight full patches, every colour, dofs of multiplicity 8
    (2, 4, (5, 3, 19)),  # every patch cut short, slots past the patch's cells
    (1, 2, (8, 8, 32)),  # eight full patches of 256 cells, items of seven cells, the flat G layout
    (1, 2, (5, 3, 19)),
    (3, 6, (2, 4, 8)),   # one cell per item, 49 of 64 lanes
    (1, 3, (4, 4, 8)),
]
# name: (mesh map, coloured plan, per-cell kappa, affine mode, Dirichlet markers)
VARIANTS = {
    "merged": (warp, False, False, False, True),
    "coloured": (warp, True, False, False, True),
    "twisted": (twist, True, False, False, True),
    "kappa": (warp, False, True, False, True),
    "affine": (shear, True, False, True, True),
    "no_markers": (warp, False, False, False, False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("pc,pf,n", SHAPES)
def test_fused_kernel_against_oracle_and_unfused_sequence(pm, pc, pf, n, variant):
    from oracle import pmg_oracle as po

    wf, coloured, var_kappa, affine, markers = VARIANTS[variant]
    part = pm.BoxPartition(n, warp=wf)
    lc, lf = part.level(pc), part.level(pf)
    bcm = lf.bc_marker if markers else np.zeros_like(lf.bc_marker)
    kappa = 0.5 + np.random.default_rng(5).random(lf.dofmap.shape[0]) if var_kappa else 2.0
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    try:
        pm.set_merge_threshold(0 if coloured else -1)
        fop = pm.MatFreeLaplacian(pf, kappa, lf.dofmap, part.xgeom, part.geom_dofmap, lf.lcells, lf.bcells, bcm, Lf)
    finally:
        pm.set_merge_threshold(-1)
    # (the small meshes merge their colours by default; threshold 0 keeps the coloured launches)
    assert fop.launches_per_apply() > 2 if coloured else fop.launches_per_apply() <= 2
    if affine:
        fop.set_geometry_mode("affine")
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    A = po.Laplacian(pf, kappa, lf.dofmap, part.xgeom, part.geom_dofmap, bcm)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    rng = np.random.default_rng(100 * pc + pf + len(variant))
    zu, ru = rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)  # non-zero on the Dirichlet dofs too
    ref = oi.reverse_interpolate(ru - A.apply(zu))
    z, r, q, coarse = _vec(pm, Lf, zu), _vec(pm, Lf, ru), pm.Vector(Lf), pm.Vector(Lc)
    q.set(float("nan"))  # the vector the unfused sequence writes A z to: the fused call never sees it
    coarse.set(3.0)      # overwritten, whatever it held
    for rep in range(2):  # the second call: no dependence on what the first left behind
        ip.restrict_residual(fop, z, r, coarse)
        got = coarse.data_copy()
        err = _relerr(got, ref)
        print(f"fused ({pc},{pf}) {n} {variant} call {rep}: rel.err vs oracle {err:.3e}")
        assert err < 1e-12
    assert np.array_equal(z.data_copy(), zu) and np.array_equal(r.data_copy(), ru)  # no fine vector is written
    assert np.isnan(q.data_copy()).all()
    # the library's own unfused sequence: q = A z, then the restriction of r - q
    fop(z, q)
    d = pm.Vector(Lf)
    d.data.copy_(r.data - q.data)
    c2 = pm.Vector(Lc)
    ip.reverse_interpolate(d, c2)
    err2 = _relerr(got, c2.data_copy())
    print(f"fused ({pc},{pf}) {n} {variant}: rel.err vs unfused sequence {err2:.3e}")
    assert err2 < 1e-12


CYCLES = [((1, 2, 4), (4, 4, 16)), ((1, 2, 4), (5, 3, 19)), ((1, 3, 6), (2, 4, 8))]


@pytest.fixture(scope="module")
def oracle_cycles():
    """Three V-cycles from zero on the numpy oracle, computed once per mesh and shared."""
    cache = {}

    def get(orders, n, eig_ranges):
        from oracle import pmg_oracle as po

        if (orders, n) not in cache:
            mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=3, warp=warp)
            for s, e in zip(sm, eig_ranges):  # the device's smoother bounds: only the cycle's arithmetic is compared
                s.eig_range = e
            xo, its = np.zeros_like(b), []
            for _ in range(3):
                xo = mg.apply(b, xo)
                its.append(xo.copy())
            cache[(orders, n)] = its
        return cache[(orders, n)]

    return get


def _cycles(h, k=3):
    x = h.new_vector()
    x.set(0.0)
    out = []
    for _ in range(k):
        h.mg.apply(h.rhs[-1], x)
        out.append(x.data_copy())
    return out


@pytest.mark.parametrize("orders,n", CYCLES)
def test_cycle_with_fused_restriction(pm, oracle_cycles, orders, n):
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=3, warp=warp)
    L = len(orders)
    ref = oracle_cycles(orders, n, h.eig_ranges)
    launches = h.operators[-1].launches_per_apply()
    h.mg.set_graph(False)
    fused = _cycles(h)
    assert h.mg.fused_restrictions() == L - 1
    counts_on = h.mg.apply_counts()
    for c, (got, want) in enumerate(zip(fused, ref)):
        err = _relerr(got, want)
        print(f"cycle {orders} {n} fused, cycle {c}: rel.err vs oracle {err:.3e}")
        assert err < 1e-10
    h.mg.set_fused_restriction(0)
    plain = _cycles(h)
    assert h.mg.fused_restrictions() == 0
    assert h.mg.apply_counts() == counts_on
    for got, want in zip(plain, ref):
        assert _relerr(got, want) < 1e-10
    for c, (a, b) in enumerate(zip(fused, plain)):
        err = _relerr(a, b)
        print(f"cycle {orders} {n}, cycle {c}: fused vs unfused {err:.3e}")
        assert err < 1e-12
    # replayed as a graph: the switch is part of the graph's key
    h.mg.set_fused_restriction(None)
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    replayed = _cycles(h)
    assert h.mg.graph_replays() == n0 + 3 and h.mg.fused_restrictions() == L - 1
    assert h.mg.apply_counts() == counts_on
    h.mg.set_fused_restriction(0)
    replayed_plain = _cycles(h)
    assert h.mg.graph_replays() == n0 + 6 and h.mg.fused_restrictions() == 0
    for a, b, e in zip(replayed, replayed_plain, fused):
        assert _relerr(a, b) < 1e-12 and _relerr(a, e) < 1e-12
    h.mg.set_graph(False)
    assert h.operators[-1].launches_per_apply() == launches


def _refused(pm, ip, op, Lf, Lc, match):
    z, r, c = pm.Vector(Lf), pm.Vector(Lf), pm.Vector(Lc)
    z.set(1.0)
    r.set(1.0)
    with pytest.raises(RuntimeError, match=match):
        ip.restrict_residual(op, z, r, c)


def test_fall_back_level_matrix_on_the_fine_level(pm, oracle_cycles):
    """An assembled matrix on the fine level: that level's applications are the matrix's, so its restriction is not
    fused; the level below still is.  (The direct entry point takes an interpolator and an operator and knows of no
    level matrix: there is nothing for it to refuse here.)"""
    orders, n = (1, 2, 4), (4, 4, 16)
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=3, warp=warp, assembled_levels=(2,))
    got = _cycles(h)
    assert h.mg.fused_restrictions() == 1
    for a, b in zip(got, oracle_cycles(orders, n, h.eig_ranges)):
        assert _relerr(a, b) < 1e-10
    h.mg.set_level_matrix(2, None)
    _cycles(h, 1)
    assert h.mg.fused_restrictions() == 2


def test_fall_back_batched_geometry(pm, oracle_cycles):
    from pmg_dolfinx_amd import _lib

    orders, n = (1, 2, 4), (4, 4, 16)
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=3, warp=warp)
    fop = h.operators[-1]
    _lib.call("pmg_laplacian_set_geometry_batch", fop.handle, 64)
    try:
        got = _cycles(h)
        assert h.mg.fused_restrictions() == 1  # the level below has its tensor resident
        for a, b in zip(got, oracle_cycles(orders, n, h.eig_ranges)):
            assert _relerr(a, b) < 1e-10
        _refused(pm, h.interpolators[-1], fop, h.layouts[-1], h.layouts[-2], "not available")
    finally:
        _lib.call("pmg_laplacian_set_geometry_batch", fop.handle, 0)
    _cycles(h, 1)
    assert h.mg.fused_restrictions() == 2


def test_fall_back_pair_without_a_kernel(pm):
    """Pair (2, 5): degree 5 is a shared-item degree, there is no fused kernel for it."""
    from oracle import pmg_oracle as po

    orders, n = (2, 5), (2, 2, 7)
    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=3, warp=warp)
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=3, warp=warp)
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    xo = np.zeros_like(b)
    for got in _cycles(h):
        xo = mg.apply(b, xo)
        assert _relerr(got, xo) < 1e-10
    assert h.mg.fused_restrictions() == 0
    _refused(pm, h.interpolators[0], h.operators[1], h.layouts[1], h.layouts[0], "not available")
    # an interpolator without the operator's patches, and an operator that is not the interpolator's
    lc, lf = h.levels
    cell_form = pm.Interpolator(2, 5, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, h.layouts[0], h.layouts[1])
    _refused(pm, cell_form, h.operators[1], h.layouts[1], h.layouts[0], "not available")


def _ghosted_body(rank, world, port):
    """One rank as its own halo partner (tests/test_gpu_distributed.py): every level's layout has ghosts, so nothing
    is fused and the cycle is the one the switch turned off gives; the direct entry point refuses.  (The
    numbers of this glued arrangement are not a mesh's solution, so there is no oracle for it; ghosted layouts are
    held to the oracle by tests/test_gpu_distributed.py, which now runs the library with the switch at its default.)"""
    import torch

    import pmg_dolfinx_amd as pm
    from pmg_dolfinx_amd import problem

    torch.cuda.set_device(0)
    native = pm.RcclComm(0, 1, pm.RcclComm.unique_id(), halo="exchange")
    orig = problem.make_layout

    def make(lv, group=None, device="cuda", comm=None):
        m = min(sum(lv.send_counts), sum(lv.recv_counts))
        si, ri = np.asarray(lv.send_indices[:m]), np.asarray(lv.recv_indices[:m])
        return pm.Layout(lv.size_local, lv.num_ghosts, [0] if m else [], [m] if m else [], [m] if m else [], si, ri,
                         device=device, comm=native)

    out = {}
    try:
        problem.make_layout = make
        H = pm.PoissonHierarchy((4, 4, 8), (1, 2, 4), cheb_its=3, proc_dims=(1, 1, 2), rank=0, size=2)
        out["ghosts"] = [lv.num_ghosts for lv in H.levels]
        H.mg.set_graph(False)
        a = _cycles(H, 2)
        out["fused"] = H.mg.fused_restrictions()
        H.mg.set_fused_restriction(0)
        b = _cycles(H, 2)
        out["diff"] = float(max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a, b)))
        z, r, c = H.new_vector(), H.new_vector(), H.new_vector(1)
        try:
            H.interpolators[-1].restrict_residual(H.operators[-1], z, r, c)
            out["refused"] = ""
        except RuntimeError as e:
            out["refused"] = str(e)
    finally:
        problem.make_layout = orig
    return out


def _ghosted_worker(rank, world, port, *rest):
    from test_gpu_distributed import _reporting

    _reporting(_ghosted_body)(rank, world, port, *rest)


def test_fall_back_layout_with_ghosts(pm):
    from test_gpu_distributed import _run_ranks

    (out,) = _run_ranks(_ghosted_worker, 1, ())
    assert all(g > 0 for g in out["ghosts"])
    assert out["fused"] == 0 and out["diff"] < 1e-12  # (the same kernels twice: atomic-order noise only)
    assert "not available" in out["refused"]
