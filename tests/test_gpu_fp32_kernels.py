"""The FP32 kernels branch by branch: the stiffness apply (laplacian_f32.hip) at full and cut-short patches, with the
streamed tensor, per-cell kappa, odd little meshes and operators not in their default state; kappa changed in place;
the patch-form transfers (the float instantiation of interpolate.hip's two patch kernels) at every degree pair through
their own entry points, and in both precisions with workgroups too small for their lists; the FP32 V-cycle (the float
instantiation of the smoother loop and passes, solvers.hip and vector.hip) at every Chebyshev degree count and with the
Krylov and callback coarse solvers; PCG with the FP32 cycle at full size.

Every FP32 output is filled with NaN before the call, so a value the kernel was meant to overwrite and did not fails
the comparison.  References: the FP64 oracles (pmg_oracle, and the C oracle at the large sizes) on the float-rounded
inputs; the cycles with Krylov or callback coarse solvers against the library's FP64 cycle.  Each tolerance is about
ten times the largest error observed on an MI355X (noted next to it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# largest error seen per tolerance class in this process (read when the tolerances are re-measured)
OBSERVED = {}

# relative errors in the max norm against the FP64 references
TOL_APPLY = 3e-6  # the float apply (observed on an MI355X: 2.8e-7)
TOL_APPLY_STREAMED = 6e-7  # ... the streamed-tensor sizes (observed 6.3e-8)
TOL_TRANSFER = 2.5e-6  # prolongation-add, restriction with and without fine_sub (observed 2.4e-7)
TOL_TRANSPOSE = 1.3e-8  # |uf . P uc - R uf . uc| over the magnitude of the two sums (observed 1.3e-9 .. 1.7e-9)
TOL_CYCLE_ORACLE = 1.8e-6  # the FP32 cycle against the oracle's FP64 cycle (observed 1.8e-7)
TOL_CYCLE_KAPPA = 1.2e-6  # ... against the library's FP64 cycle after kappa changed in place (observed 1.2e-7)
TOL_CYCLE_COARSE = 1.2e-5  # ... with a Krylov or callback coarse solver (observed 1.2e-6)


def _check(what, err, tol):
    OBSERVED[what] = max(OBSERVED.get(what, 0.0), float(err))
    assert err < tol, (what, err, tol)


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _f32(a):
    """The float rounding of a host array, back in FP64 (the input the FP32 kernels see)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _nan32(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


def _apply32(op, u, x=None):
    """y = A u in FP32 into a NaN-filled output."""
    x = _dev32(u) if x is None else x
    y = _nan32(x.numel())
    op.apply_fp32(x, y)
    return _host(y)


def _check_apply(op, u, ref, bc, what="apply", tol=TOL_APPLY, reps=2):
    """`reps` applications in a row, each against the oracle; Dirichlet rows exactly float(u)."""
    x = _dev32(u)
    m = np.asarray(bc).astype(bool)
    for _ in range(reps):
        got = _apply32(op, u, x)
        _check(what, _relerr(got, ref), tol)
        assert np.array_equal(got[m], _f32(u[m]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the stiffness apply
# ---------------------------------------------------------------------------------------------------------------------

# the shapes of test_gpu_parity.py::test_apply_parity_full_patches: every patch full (tensor grid: the structured patch
# builder), then meshes whose patches are all cut short
FULL_PATCHES = [(1, (8, 8, 16)), (2, (4, 4, 16)), (3, (4, 4, 8)), (4, (4, 4, 8)), (5, (4, 4, 14)), (6, (2, 4, 8)),
                (7, (2, 2, 6)), (8, (2, 2, 6)), (5, (4, 4, 4)), (6, (2, 4, 4)), (7, (2, 2, 4)), (8, (2, 2, 8))]


def _operator(pm, P, kappa, lv, part, bcm, layout, merge=None, **kw):
    if merge is not None:
        pm.set_merge_threshold(merge)
    try:
        return pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bcm,
                                   layout, **kw)
    finally:
        pm.set_merge_threshold(-1)


@pytest.mark.parametrize("merge", [0, 1 << 40], ids=["coloured", "merged"])
@pytest.mark.parametrize("P,n", FULL_PATCHES)
def test_fp32_apply_full_patches(pm, P, n, merge):
    from oracle import pmg_oracle as po

    part = pm.BoxPartition(n)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    op = _operator(pm, P, 2.0, lv, part, lv.bc_marker, layout, merge)
    if merge != 0:
        assert op.launches_per_apply() == 1
    A = po.Laplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker)
    if (P, n) in ((2, (4, 4, 16)), (4, (4, 4, 8))):
        # the profile counts the kernel launches the FP32 walk of the plan issued
        op.set_profiling(True)
        _apply32(op, u)
        assert op.read_profile()[1] == op.launches_per_apply()
        op.set_profiling(False)


# the smallest cube whose float tensor (24 B per quadrature point) is past the 128 MiB above which the kernel streams it
# with non-temporal loads and stores (laplacian_f32.hip, laplacian_apply_f32)
STREAMED = {2: 60, 3: 45, 4: 36, 5: 30, 6: 26, 7: 23, 8: 20}


@pytest.mark.parametrize("P", sorted(STREAMED))
def test_fp32_apply_streamed_tensor(pm, P):
    """Production sizes take the streamed form; in a coloured plan colour c + 1 gathers what colour c stored with
    non-temporal stores."""
    from oracle import c_oracle as co

    n = STREAMED[P]
    assert 24 * n**3 * (P + 1) ** 3 > 128 << 20  # (the test stays on the streamed form if the threshold stays)
    part = pm.BoxPartition(n)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    A = co.CLevel(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    ref = A.apply(_f32(u))
    for merge in (0, 1 << 40):
        op = _operator(pm, P, 2.0, lv, part, lv.bc_marker, layout, merge)
        if merge == 0:
            assert op.launches_per_apply() > 1
        _check_apply(op, u, ref, lv.bc_marker, "apply_streamed", TOL_APPLY_STREAMED)
        del op
        torch.cuda.empty_cache()


@pytest.mark.parametrize("contrast", [False, True], ids=["uniform", "contrast1e3"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_apply_per_cell_kappa(pm, P, contrast):
    from oracle import pmg_oracle as po

    rng = np.random.default_rng(300 + P)
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    if contrast:
        kappa = np.where(rng.uniform(size=part.ncells) < 0.5, 1e-3, 1.0) * rng.uniform(1.0, 2.0, part.ncells)
    else:
        kappa = rng.uniform(0.5, 3.0, part.ncells)
    A = po.Laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = rng.standard_normal(lv.ndofs)
    ref = A.apply(_f32(u))
    for merge in (0, 1 << 40):
        op = _operator(pm, P, kappa, lv, part, lv.bc_marker, layout, merge)
        _check_apply(op, u, ref, lv.bc_marker)


def test_fp32_apply_random_small_meshes(pm):
    """test_gpu_parity.py::test_apply_parity_random_small_meshes in FP32: odd little meshes, an arbitrary split into
    the two cell lists, a random Dirichlet marker, per-cell kappa."""
    from oracle import pmg_oracle as po

    rng = np.random.default_rng(2025)
    shapes = [(1, 1, 1), (1, 1, 9), (9, 1, 1), (2, 3, 1), (1, 5, 2), (3, 3, 3), (5, 2, 7), (4, 4, 9)]
    for case in range(24):
        P = int(rng.integers(1, 9))
        n = shapes[case % len(shapes)] if P <= 4 else shapes[case % 6]
        part = pm.BoxPartition(n, warp=twist)
        lv = part.level(P)
        bc = (rng.uniform(size=lv.ndofs) < 0.15).astype(np.int8)
        kappa = rng.uniform(0.5, 2.0, part.ncells)
        mask = rng.uniform(size=part.ncells) < 0.6
        lcells = np.nonzero(mask)[0].astype(np.int32)
        bcells = np.nonzero(~mask)[0].astype(np.int32)
        layout = pm.Layout(lv.ndofs)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lcells, bcells, bc, layout)
        A = po.Laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, bc)
        u = rng.standard_normal(lv.ndofs)
        _check_apply(op, u, A.apply(_f32(u)), bc)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_apply_basix_node_order(pm, P):
    from oracle import pmg_oracle as po

    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    dm_basix = pm.dofmap_in_node_order(lv.dofmap, pm.basix_node_permutation(P))
    op = pm.MatFreeLaplacian(P, 2.0, dm_basix, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout, node_order="basix")
    A = po.Laplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(40 + P).standard_normal(lv.ndofs)
    _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker)


@pytest.mark.parametrize("P,pc", [(1, None), (2, 1), (3, None), (4, 2), (6, 3), (8, 4)])
def test_fp32_irregular_numbering(pm, P, pc):
    """test_gpu_parity.py::test_irregular_numbering in FP32: cells in arbitrary order, dofs renumbered, vertices
    jittered (Morton-chunk patches closed early), per-cell kappa; apply and the two transfers."""
    from oracle import pmg_oracle as po

    rng = np.random.default_rng(1000 + P)
    n = (5, 4, 6) if P <= 4 else (3, 2, 3)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(P)
    ncells, ndofs = part.ncells, lv.ndofs
    x = part.xgeom.copy()
    h = 1.0 / max(n)
    inner = np.all((x > 1e-9) & (x < 1 + 0.3), axis=1)
    x[inner] += 0.08 * h * rng.uniform(-1, 1, (int(inner.sum()), 3))
    cperm = rng.permutation(ncells)
    dperm = rng.permutation(ndofs)
    dofmap = dperm[lv.dofmap[cperm]].astype(np.int32)
    gdm = part.geom_dofmap[cperm]
    bc = np.zeros(ndofs, dtype=np.int8)
    bc[dperm] = lv.bc_marker
    kappa = rng.uniform(0.5, 3.0, ncells)
    mask = rng.uniform(size=ncells) < 0.7
    lcells, bcells = np.nonzero(mask)[0].astype(np.int32), np.nonzero(~mask)[0].astype(np.int32)
    layout = pm.Layout(ndofs)
    op = pm.MatFreeLaplacian(P, kappa, dofmap, x, gdm, lcells, bcells, bc, layout)
    A = po.Laplacian(P, kappa, dofmap, x, gdm, bc)
    u = rng.standard_normal(ndofs)
    _check_apply(op, u, A.apply(_f32(u)), bc)
    if pc is None:
        return
    lvc = part.level(pc)
    cdperm = rng.permutation(lvc.ndofs)
    dmc = cdperm[lvc.dofmap[cperm]].astype(np.int32)
    Lc = pm.Layout(lvc.ndofs)
    ip = pm.Interpolator(pc, P, dmc, dofmap, lcells, bcells, Lc, layout, fine_operator=op)
    oi = po.Interpolator(pc, P, dmc, dofmap, lvc.ndofs, ndofs)
    _check_transfers(ip, oi, lvc.ndofs, ndofs, rng)


def test_fp32_apply_affine_geometry_mode(pm):
    """The float form always streams its stored tensor: an operator switched to the affine mode gives the same FP32
    apply."""
    from oracle import pmg_oracle as po

    shear = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])
    for P in range(1, 9):
        n = (4, 4, 8) if P <= 4 else (2, 2, 4)
        part = pm.BoxPartition(n, warp=lambda x: x @ shear.T)
        lv = part.level(P)
        layout = pm.make_layout(lv)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                 lv.bc_marker, layout)
        assert op.is_affine()
        op.set_geometry_mode("affine")
        A = po.Laplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
        u = np.random.default_rng(P).standard_normal(lv.ndofs)
        _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker)


@pytest.mark.parametrize("n", [(4, 4, 64), (4, 4, 19)])
def test_fp32_apply_chain_form(pm, n, monkeypatch):
    """Degree 4 with the chain form on (the FP64 apply's interior as chains of patches): the FP32 apply keeps the
    patch plan and still gives the oracle's vector."""
    from oracle import c_oracle as co

    P = 4
    part = pm.BoxPartition(n)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    monkeypatch.setenv("PMG_CHAIN", "2")
    op = _operator(pm, P, 2.0, lv, part, lv.bc_marker, layout, 0)
    op.set_chain_form(True)
    assert op.chain_form()
    A = co.CLevel(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker)


@pytest.mark.parametrize("P,n", [(2, (16, 8, 32)), (4, (8, 6, 32)), (6, (4, 4, 32)), (8, (8, 2, 12))])
def test_fp32_apply_two_stream_plan(pm, P, n, monkeypatch):
    from oracle import c_oracle as co

    part = pm.BoxPartition(n, warp=lambda x: x + 0.05 * np.sin(2.0 * np.pi * x))
    lv = part.level(P)
    layout = pm.make_layout(lv)
    monkeypatch.setenv("PMG_APPLY_STREAMS", "2")
    op = _operator(pm, P, 2.0, lv, part, lv.bc_marker, layout, 0)
    assert op.apply_streams() == 2
    A = co.CLevel(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(11).standard_normal(lv.ndofs)
    _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_apply_uncovered_dofs(pm, P):
    """Cell lists that leave dofs of the layout in no listed cell: those rows are zero (Dirichlet ones as well: no
    cell writes them)."""
    from oracle import pmg_oracle as po

    rng = np.random.default_rng(500 + P)
    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=twist)
    lv = part.level(P)
    keep = np.sort(rng.permutation(part.ncells)[: part.ncells // 2])
    lcells = keep[: len(keep) // 2].astype(np.int32)
    bcells = keep[len(keep) // 2:].astype(np.int32)
    layout = pm.make_layout(lv)
    kappa = rng.uniform(0.5, 3.0, part.ncells)
    op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lcells, bcells, lv.bc_marker,
                             layout)
    A = po.Laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    u = rng.standard_normal(lv.ndofs)
    ref = A.apply(_f32(u), cells=keep)
    touched = np.zeros(lv.ndofs, dtype=bool)
    touched[lv.dofmap[keep].ravel()] = True
    assert not touched.all()
    _check_apply(op, u, ref, lv.bc_marker.astype(bool) & touched)
    got = _apply32(op, u)
    assert np.all(got[~touched] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. kappa changed in place
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_apply_reads_kappa_in_every_application(pm, P):
    from oracle import pmg_oracle as po

    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    part = pm.BoxPartition(n, warp=warp)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    kappa = torch.full((part.ncells,), 2.0, dtype=torch.float64, device="cuda")
    op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    A = po.Laplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    _check_apply(op, u, A.apply(_f32(u)), lv.bc_marker, reps=1)
    kappa[: part.ncells // 2] *= 10.0
    A2 = po.Laplacian(P, kappa.cpu().numpy(), lv.dofmap, part.xgeom, part.geom_dofmap, lv.bc_marker)
    _check_apply(op, u, A2.apply(_f32(u)), lv.bc_marker, reps=1)


def test_fp32_cycle_after_kappa_changed_in_place(pm):
    """PoissonHierarchy.kappa changed in place and every diagonal recomputed: the FP32 cycle is still the FP64 cycle
    to float rounding, eager and replayed from a graph captured before the change."""
    h = pm.PoissonHierarchy(4, (1, 2, 4), kappa=2.0, cheb_its=3, warp=warp)
    b = h.rhs[-1]
    x = h.new_vector()

    def cycle(prec, graph):
        h.mg.set_precision(prec)
        h.mg.set_graph(graph)
        x.set(0.0)
        h.mg.apply(b, x)
        return x.data_copy()

    cycle("fp32", False)
    cycle("fp32", True)  # captured with the first kappa
    n0 = h.mg.graph_replays()
    cycle("fp32", True)
    assert h.mg.graph_replays() > n0
    h.kappa[: h.kappa.numel() // 2] *= 10.0
    for op in h.operators:
        op.compute_diag_inverse()
    ref = cycle("fp64", False)
    _check("cycle_kappa", _relerr(cycle("fp32", False), ref), TOL_CYCLE_KAPPA)
    _check("cycle_kappa", _relerr(cycle("fp32", True), ref), TOL_CYCLE_KAPPA)
    _check("cycle_kappa", _relerr(cycle("fp32", True), ref), TOL_CYCLE_KAPPA)
    h.mg.set_graph(False)
    h.mg.set_precision("fp64")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the transfers
# ---------------------------------------------------------------------------------------------------------------------

def _check_transfers(ip, oi, nc, nf, rng):
    """prolongation-add, restriction with and without fine_sub (twice, into NaN), the transpose identity; against
    the FP64 oracle on the float-rounded inputs."""
    uc, uf, us = _f32(rng.standard_normal(nc)), _f32(rng.standard_normal(nf)), _f32(rng.standard_normal(nf))
    vc, vf, vs = _dev32(uc), _dev32(uf), _dev32(us)
    fine = vf.clone()
    ip.interpolate_add_fp32(vc, fine)
    _check("prolong_add", _relerr(_host(fine), uf + oi.interpolate(uc)), TOL_TRANSFER)
    pz = torch.zeros_like(vf)
    ip.interpolate_add_fp32(vc, pz)
    Puc = _host(pz)
    _check("prolong_add", _relerr(Puc, oi.interpolate(uc)), TOL_TRANSFER)
    ref = oi.reverse_interpolate(uf)
    for _ in range(2):
        coarse = _nan32(nc)
        ip.reverse_interpolate_fp32(vf, coarse)
        Ruf = _host(coarse)
        _check("restrict", _relerr(Ruf, ref), TOL_TRANSFER)
    ref_d = oi.reverse_interpolate(uf - us)
    for _ in range(2):
        coarse = _nan32(nc)
        ip.reverse_interpolate_fp32(vf, coarse, fine_sub=vs)
        _check("restrict_difference", _relerr(_host(coarse), ref_d), TOL_TRANSFER)
    # restriction is the transpose of prolongation, to float rounding of the two float results
    scale = np.abs(uf).max() * np.abs(Puc).sum() + np.abs(uc).max() * np.abs(Ruf).sum()
    _check("transpose", abs(uf @ Puc - Ruf @ uc) / scale, TOL_TRANSPOSE)


PAIRS = [(pc, pf) for pf in range(2, 9) for pc in range(1, pf)]
# the full and cut-short shapes of test_gpu_parity.py::test_transfer_parity
TRANSFER_SHAPES = [(2, 4, (4, 4, 16), False), (1, 2, (4, 4, 16), False), (1, 4, (2, 4, 8), False),
                   (2, 5, (2, 2, 7), True), (2, 5, (2, 2, 4), False), (3, 7, (2, 2, 6), True),
                   (3, 6, (2, 2, 8), False), (4, 8, (2, 2, 6), False)]


def _transfer_case(pm, pc, pf, n, warped):
    from oracle import pmg_oracle as po

    part = pm.BoxPartition(n, warp=warp if warped else None)
    lc, lf = part.level(pc), part.level(pf)
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    fop = pm.MatFreeLaplacian(pf, 2.0, lf.dofmap, part.xgeom, part.geom_dofmap, lf.lcells, lf.bcells, lf.bc_marker,
                              Lf)
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    _check_transfers(ip, oi, lc.ndofs, lf.ndofs, np.random.default_rng(pc * 10 + pf))


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_fp32_transfers_every_pair(pm, pc, pf):
    assert len(PAIRS) == 28
    _transfer_case(pm, pc, pf, (3, 2, 2), True)


@pytest.mark.parametrize("pc,pf,n,warped", TRANSFER_SHAPES)
def test_fp32_transfers_full_and_cut_short_patches(pm, pc, pf, n, warped):
    _transfer_case(pm, pc, pf, n, warped)


TOL_TRANSFER_FP64 = 1e-12  # the FP64 transfers against the oracle (test_gpu_parity.py::test_transfer_parity)


# (coarse degree, fine degree, cells of the box, cells of one patch of the fine operator: patch_shape(), patches.hpp)
FEW_WAVEFRONT_CASES = [(1, 2, (4, 4, 16), (4, 4, 16)), (2, 4, (4, 4, 8), (2, 2, 8))]


@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("pc,pf,n,block", FEW_WAVEFRONT_CASES)
def test_transfers_with_few_wavefronts(pm, pc, pf, n, block, waves, monkeypatch):
    """PMG_TRANSFER_WAVES (read when the interpolator is created) makes the workgroup smaller than its patch's lists:
    the fine list of a patch is longer than the 6 entries per thread the prolongation holds in registers (its tail
    loop) and the coarse list longer than the workgroup (the restriction's loops behind the first entry per thread).
    Both boxes are whole patches of the fine operator on a tensor grid (the structured builder: full blocks, checked
    on the host by test_patch_plans.py), so every patch has (pf bx + 1)(pf by + 1)(pf bz + 1) = 2 673 fine and
    (pc bx + 1)(pc by + 1)(pc bz + 1) = 425 coarse dofs: one patch for (1, 2), four for (2, 4).  Both precisions of
    the same two kernels."""
    assert all(m % b == 0 for m, b in zip(n, block))  # whole patches only
    fine_list = int(np.prod([pf * b + 1 for b in block]))
    coarse_list = int(np.prod([pc * b + 1 for b in block]))
    assert (fine_list, coarse_list) == (2673, 425)
    assert fine_list > 6 * 64 * waves and coarse_list > 64 * waves  # TRANSFER_LIST_ITER x threads; threads
    from oracle import pmg_oracle as po

    monkeypatch.setenv("PMG_TRANSFER_WAVES", str(waves))
    part = pm.BoxPartition(n)
    lc, lf = part.level(pc), part.level(pf)
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    fop = pm.MatFreeLaplacian(pf, 2.0, lf.dofmap, part.xgeom, part.geom_dofmap, lf.lcells, lf.bcells, lf.bc_marker,
                              Lf)
    ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf, fine_operator=fop)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    rng = np.random.default_rng(waves * 100 + pc * 10 + pf)
    uc, uf = rng.standard_normal(lc.ndofs), rng.standard_normal(lf.ndofs)

    def vec(layout, values):
        v = pm.Vector(layout)
        v.data.copy_(torch.from_numpy(values))
        return v

    vc, vf = vec(Lc, uc), vec(Lf, np.full(lf.ndofs, np.nan))
    ip.interpolate(vc, vf)
    _check("fp64_prolong", _relerr(vf.data_copy(), oi.interpolate(uc)), TOL_TRANSFER_FP64)
    vf = vec(Lf, uf)
    ip.interpolate_add(vc, vf)
    _check("fp64_prolong_add", _relerr(vf.data_copy(), uf + oi.interpolate(uc)), TOL_TRANSFER_FP64)
    vf, vc = vec(Lf, uf), vec(Lc, np.full(lc.ndofs, np.nan))
    ip.reverse_interpolate(vf, vc)
    _check("fp64_restrict", _relerr(vc.data_copy(), oi.reverse_interpolate(uf)), TOL_TRANSFER_FP64)
    _check_transfers(ip, oi, lc.ndofs, lf.ndofs, rng)


def test_fp32_transfer_refusals(pm):
    from pmg_dolfinx_amd import _lib

    part = pm.BoxPartition((2, 2, 2))
    lc, lf = part.level(1), part.level(2)
    Lc, Lf = pm.make_layout(lc), pm.make_layout(lf)
    ip = pm.Interpolator(1, 2, lc.dofmap, lf.dofmap, lf.lcells, lf.bcells, Lc, Lf)  # cell form
    with pytest.raises(_lib.PmgError, match="patch-form"):
        ip.interpolate_add_fp32(_nan32(lc.ndofs), _nan32(lf.ndofs))
    with pytest.raises(_lib.PmgError, match="patch-form"):
        ip.reverse_interpolate_fp32(_nan32(lf.ndofs), _nan32(lc.ndofs))
    with pytest.raises(TypeError):
        ip.reverse_interpolate_fp32(torch.zeros(lf.ndofs, dtype=torch.float64, device="cuda"), _nan32(lc.ndofs))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the FP32 cycle
# ---------------------------------------------------------------------------------------------------------------------

CYCLE_HIERARCHIES = [((3,), 3), ((1, 5), (2, 2, 7)), ((3, 7), (2, 2, 3)), ((1, 2, 4, 8), 3), ((2, 4), (3, 4, 2))]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("orders,n", CYCLE_HIERARCHIES)
def test_fp32_cycle_against_fp64_oracle(pm, orders, n, k):
    """One cycle from zero and one from a non-zero guess; k = 1 and 2 take the short branches of the FP32 Chebyshev
    (one step: no fused update; two: the last step drops r and z)."""
    from oracle import pmg_oracle as po

    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=k, warp=warp)
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=k, warp=warp)
    for s_, e in zip(sm, h.eig_ranges):
        s_.eig_range = e
    h.mg.set_precision("fp32")
    rng = np.random.default_rng(17 * k + len(orders))
    r = rng.standard_normal(b.size)
    if len(orders) == 1:
        # one level: the library smooths the caller's rhs as it is (FP64 alike), the reference masks the Dirichlet
        # rows of the coarsest rhs first
        r[mesh.boundary_marker(orders[0]).astype(bool)] = 0.0
    x = h.new_vector()
    x.set(0.0)
    rv = pm.Vector(h.layouts[-1])
    rv.data.copy_(torch.from_numpy(r))
    h.mg.apply(rv, x)
    _check("cycle_oracle", _relerr(x.data_copy(), mg.apply(r, np.zeros_like(r))), TOL_CYCLE_ORACLE)
    y0 = rng.standard_normal(b.size)
    x.data.copy_(torch.from_numpy(y0))
    h.mg.apply(rv, x)
    _check("cycle_oracle", _relerr(x.data_copy(), mg.apply(r, y0)), TOL_CYCLE_ORACLE)


class _CallbackCoarse:
    """A coarse solver the library knows nothing about: called back from inside the cycle."""

    def __init__(self, pm, op, layout):
        self.op = op
        self.cg = pm.CGSolver(layout)
        self.cg.set_max_iterations(10)
        self.cg.set_tolerance(0.0)

    def solve(self, x, b):
        x.set(0.0)
        self.cg.solve(self.op, x, b)


@pytest.mark.parametrize("coarse", ["cg", "callback"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_fp32_cycle_with_krylov_and_callback_coarse_solvers(pm, coarse, k):
    h = pm.PoissonHierarchy(6, (1, 2, 4), kappa=2.0, cheb_its=k, warp=warp)
    if coarse == "cg":
        solver = pm.CGSolver(h.layouts[0])
        solver.set_max_iterations(10)
        solver.set_tolerance(0.0)
    else:
        solver = _CallbackCoarse(pm, h.operators[0], h.layouts[0])
    h.mg.set_coarse_solver(solver)
    b = h.rhs[-1]
    y0 = np.random.default_rng(k).standard_normal(b.data.numel())
    out = {}
    for prec in ("fp64", "fp32"):
        h.mg.set_precision(prec)
        x = h.new_vector()
        x.set(0.0)
        h.mg.apply(b, x)
        x2 = h.new_vector()
        x2.data.copy_(torch.from_numpy(y0))
        h.mg.apply(b, x2)
        out[prec] = (x.data_copy(), x2.data_copy())
    _check("cycle_coarse", _relerr(out["fp32"][0], out["fp64"][0]), TOL_CYCLE_COARSE)
    _check("cycle_coarse", _relerr(out["fp32"][1], out["fp64"][1]), TOL_CYCLE_COARSE)
    h.mg.set_coarse_solver(None)


# ---------------------------------------------------------------------------------------------------------------------
# 5. full size
# ---------------------------------------------------------------------------------------------------------------------

def test_fp32_pcg_full_size(pm):
    """64^3, p = 4 -> 2 -> 1, AMG coarse solver: PCG with the FP32 cycle takes at most one more iteration than with
    the FP64 one and reaches the same true residual (the streamed float tensor on the two finer levels)."""
    h = pm.PoissonHierarchy(64, (1, 2, 4), kappa=2.0, cheb_its=3)
    h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], cycles=2))

    def pcg():
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(60)
        cg.set_tolerance(1e-8)
        x = h.new_vector()
        x.set(0.0)
        its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
        r = pm.Vector(h.layouts[-1])
        h.operators[-1](x, r)
        pm.axpy(r, -1.0, r, h.rhs[-1])
        return its, pm.norm(r) / pm.norm(h.rhs[-1])

    its64, res64 = pcg()
    h.mg.set_precision("fp32")
    its32, res32 = pcg()
    h.mg.set_precision("fp64")
    OBSERVED["pcg_full_size"] = (its64, res64, its32, res32)
    assert its32 <= its64 + 1, (its32, its64)
    assert res32 <= 1.5 * res64, (res32, res64)
