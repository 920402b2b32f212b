"""Every connectivity-dependent path of the library on multi-block hexahedral meshes (tests/multiblock_mesh.py): stars of
3 and 5 sectors around an edge (an edge shared by 3 / 5 cells, vertices of valence 6 / 10, one Jacobian per sector, bent
into trilinear cells), the O-grid (edges of 3 cells, vertices of valence 3, 4 and 6, left-handed blocks, twisted) and the
notched grid (re-entrant edges, a cavity, boundary dofs inside the bounding box).  The reference is always the oracle, or
a tests/*_reference.py module, on the SAME arrays.  The helper and the oracles on these meshes are pinned on the CPU by
tests/test_multiblock_mesh.py, the launch plans by the ``multiblock`` group of tests/test_patch_plans.py.

Bounds are those the existing test of the same quantity asserts (test_gpu_parity.py, test_gpu_fp32_kernels.py,
test_gpu_cell_frames.py, test_gpu_amg.py, test_gpu_mixed_precision.py, test_gpu_distributed.py).  The worst observed
value per mesh and check is printed, and written as JSON to the file named by PMG_MULTIBLOCK_REPORT if that is set
(profiles/multiblock.md)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as bd  # noqa: E402
import multiblock_mesh as mb  # noqa: E402
import reaction_reference as rr  # noqa: E402
import robin_reference as rb  # noqa: E402
import tensor_coefficient_reference as tc  # noqa: E402
from boundary_data_reference import twist  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12  # FP64 apply, diagonal, load vectors, boundary terms, matrix entries (test_gpu_parity / _boundary_data)
TOL_G = 1e-13  # the exported tensor (test_gpu_parity.py::test_apply_parity_all_degrees)
TOL_PROLONG = 1e-13  # test_gpu_parity.py::test_transfer_parity
TOL_APPLY32 = 3e-6  # test_gpu_fp32_kernels.py: TOL_APPLY
TOL_TRANSFER32 = 2.5e-6  # ... TOL_TRANSFER
TOL_CYCLE32 = 1.8e-6  # ... TOL_CYCLE_ORACLE
TOL_CYCLE = 1e-10  # test_gpu_parity.py::test_vcycle_parity, test_gpu_distributed.py: vcycle_err
TOL_RNORM = 1e-9  # test_gpu_parity.py::test_vcycle_parity
TOL_GRAPH = 1e-13  # test_gpu_parity.py::test_vcycle_graph_replay
TOL_EIG = 1e-8
TOL_AMG = 1e-11  # test_gpu_amg.py::test_cycle_equals_numpy_restatement

OBSERVED = {}  # (mesh, check) -> [worst error, bound]
FORMS = {}  # mesh -> {optional form: what the library decided}


def _check(mesh, what, err, tol):
    w = OBSERVED.setdefault((mesh, what), [0.0, tol])
    w[0] = max(w[0], float(err))
    print(f"multiblock: {mesh}: {what} {err:.3e} (worst so far {w[0]:.3e}, bound {tol:.1e})")
    assert err < tol, (mesh, what, err, tol)


def _form(mesh, what, value):
    FORMS.setdefault(mesh, {}).setdefault(what, set()).add(str(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("PMG_MULTIBLOCK_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"observed": [[m, w, v[0], v[1]] for (m, w), v in sorted(OBSERVED.items())],
                       "forms": {m: {k: sorted(v) for k, v in d.items()} for m, d in FORMS.items()}}, f, indent=1)


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
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def kappa_of(ncells):
    return np.random.default_rng(3).uniform(0.5, 3.0, ncells)


def split_cells(ncells, seed=1):
    mask = np.random.default_rng(seed).uniform(size=ncells) < 0.7
    return np.nonzero(mask)[0].astype(np.int32), np.nonzero(~mask)[0].astype(np.int32)


# ---- the meshes: per degree the smallest that still holds several patches (patch_shape: 256 cells at degrees 1 and 2,
# 32 at 3 and 4, 7 / 8 / 12 / 3 at 5 / 6 / 7 / 8) -----------------------------------------------------------------------
_MESHES = {}


def _size(P):
    return "L" if P <= 2 else ("M" if P <= 4 else "S")


def mesh_of(name, size):
    """size L: a sector of 4 x 4 x 16 cells; M: 2 x 2 x 8; S: 2 x 2 x 3."""
    key = (name, size)
    if key not in _MESHES:
        m, nz, og = {"L": (4, 16, 6), "M": (2, 8, 3), "S": (2, 3, 2)}[size]
        if name == "star3":
            _MESHES[key] = mb.star(3, m, nz)
        elif name == "star5 bent":
            _MESHES[key] = mb.star(5, m, nz, bend=0.3)
        elif name == "ogrid twisted":
            _MESHES[key] = mb.ogrid(og, map=twist)
        elif name == "notched":
            _MESHES[key] = mb.notched({"L": (4, 4, 48), "M": (4, 4, 16), "S": (4, 3, 8)}[size])
        else:
            raise KeyError(name)
    return _MESHES[key]


def test_the_meshes_are_what_they_claim(pm):
    """Irregular edges and vertices, left-handed cells, a cavity: counted, not assumed."""
    t = mesh_of("star3", "S").topology()
    assert t["edge_valence"][3] == 3 and t["vertex_valence"][6] == 2
    t = mesh_of("star5 bent", "M").topology()
    assert t["edge_valence"][5] == 8 and t["vertex_valence"][10] == 7
    o = mesh_of("ogrid twisted", "S")
    assert dict(o.topology()["edge_valence"]) == {2: 48, 3: 40, 4: 114} and int(o.left_handed().sum()) == 24
    t = mesh_of("notched", "S").topology()
    assert t["V"] - t["E"] + t["F"] - t["C"] == 2 and t["edge_valence"][3] > 0


def build_op(pm, mesh, P, kappa, form, marker=None):
    """form "coloured": one cell list, every colour a launch of its own; "merged": two cell lists, the default
    threshold (levels as small as these are merged)."""
    lv = mesh.level(P)
    layout = pm.make_layout(lv)
    bc = lv.bc_marker if marker is None else np.ascontiguousarray(marker, dtype=np.int8)
    lcells, bcells = (lv.lcells, lv.bcells) if form == "coloured" else split_cells(mesh.ncells)
    try:
        if form == "coloured":
            pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lcells, bcells, bc, layout)
    finally:
        pm.set_merge_threshold(-1)
    return lv, layout, op


def check_apply64(pm, mesh, op, layout, u, ref, what="apply fp64", reps=2):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    for rep in range(reps):
        y.set(7.0 + rep)
        op(x, y)
        _check(mesh, what, _relerr(y.data_copy(), ref), TOL)


def check_apply32(mesh, op, u, ref32, bc, what="apply fp32"):
    x = _dev32(u)
    y = torch.full((x.numel(),), float("nan"), dtype=torch.float32, device="cuda")
    op.apply_fp32(x, y)
    got = _host(y)
    _check(mesh, what, _relerr(got, ref32), TOL_APPLY32)
    m = np.asarray(bc).astype(bool)
    assert np.array_equal(got[m], _f32(u[m]))


# ---------------------------------------------------------------------------------------------------------------------
# apply (FP64, FP32), inverse diagonal, load vector, exported tensor, geometry modes
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["coloured", "merged"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("name", ["star3", "star5 bent", "ogrid twisted"])
def test_apply_diagonal_rhs_geometry(pm, name, P, form):
    from oracle import pmg_oracle as po

    mesh = mesh_of(name, _size(P))
    kappa = kappa_of(mesh.ncells)
    lv, layout, op = build_op(pm, mesh, P, kappa, form)
    A = po.Laplacian(P, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.bc_marker)
    K = {1: 256, 2: 256, 3: 32, 4: 32, 5: 7, 6: 8, 7: 12, 8: 3}[P]
    assert mesh.ncells >= 3 * K
    if form == "coloured":
        assert op.launches_per_apply() >= 2  # at least three interior patches, no two of one colour adjacent
    else:
        assert op.launches_per_apply() <= 2  # one merged launch per cell list
    u = np.random.default_rng(10 + P).standard_normal(lv.ndofs)
    ref = A.apply(u)
    check_apply64(pm, name, op, layout, u, ref, what=f"apply fp64, {form}")
    check_apply32(name, op, u, A.apply(_f32(u)), lv.bc_marker, what=f"apply fp32, {form}")
    op.compute_diag_inverse()
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    _check(name, "diag_inverse", _relerr(d.data_copy(), A.diag_inverse()), TOL)
    c = mesh.dof_coordinates(P)
    fv = 29 * np.pi**2 * np.sin(2 * np.pi * c[:, 0]) * np.sin(3 * np.pi * c[:, 1]) * np.sin(4 * np.pi * c[:, 2])
    b = pm.Vector(layout)
    b.set(5.0)
    op.assemble_rhs(_vec(pm, layout, fv), b)
    _check(name, "assemble_rhs", _relerr(b.data_copy(), A.rhs_manufactured(c)), TOL)
    G = op.geometry().cpu().numpy()
    _check(name, "geometry()", _relerr(G, A.G), TOL_G)
    assert (G[:, :, [0, 3, 5]] > 0).all()  # left-handed cells included
    # sheared cells with one Jacobian per sector are affine; bent and twisted ones are not
    assert op.is_affine() == (name == "star3")
    if name == "star3":
        op.set_geometry_mode("affine")
        check_apply64(pm, name, op, layout, u, ref, what="apply fp64, affine mode")
        check_apply32(name, op, u, A.apply(_f32(u)), lv.bc_marker, what="apply fp32, affine mode")
        op.set_geometry_mode("stored")
        check_apply64(pm, name, op, layout, u, ref, what=f"apply fp64, {form}", reps=1)


@pytest.mark.parametrize("name,size", [("notched", "L"), ("star5 bent", "L"), ("ogrid twisted", "L")])
def test_two_stream_split(pm, name, size, monkeypatch):
    """PMG_APPLY_STREAMS=2 on a coloured level of more than 16 patches: the notched grid is split over two streams (as
    the host checker finds for the same cells); a star or an O-grid is split only if the colours of its Morton patches
    separate the halves (the host checker's are not); either way the product is the oracle's."""
    from oracle import c_oracle as co

    P = 4
    mesh = mb.star(5, 4, 8, bend=0.3) if name == "star5 bent" else (
        mb.ogrid(4, map=twist) if name == "ogrid twisted" else mesh_of(name, size))
    lv = mesh.level(P)
    layout = pm.make_layout(lv)
    A = co.CLevel(P, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(11).standard_normal(lv.ndofs)
    monkeypatch.setenv("PMG_APPLY_STREAMS", "2")
    try:
        pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
    finally:
        pm.set_merge_threshold(-1)
    _form(name, "two-stream split (P = 4)", "split" if op.apply_streams() == 2 else "refused, one sequence")
    if name == "notched":  # (its centroids lie on a tensor grid: the host checker's plan of the same cells is split)
        assert op.apply_streams() == 2
    assert op.launches_per_apply() >= 3
    check_apply64(pm, name, op, layout, u, A.apply(u), what="apply fp64, PMG_APPLY_STREAMS=2", reps=3)
    check_apply32(name, op, u, A.apply(_f32(u)), lv.bc_marker, what="apply fp32, PMG_APPLY_STREAMS=2")


@pytest.mark.parametrize("name", ["notched", "star3"])
def test_chain_form(pm, name, monkeypatch):
    """PMG_CHAIN=2: the chain form needs a tensor grid of patches.  Where a mesh has none the form reports itself
    unavailable before anything is launched and the patch form is the oracle's; where it has one the chain form is."""
    from oracle import c_oracle as co

    P = 4
    mesh = mesh_of(name, "L") if name == "notched" else mb.star(3, 4, 12)
    lv = mesh.level(P)
    layout = pm.make_layout(lv)
    A = co.CLevel(P, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.bc_marker)
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    monkeypatch.setenv("PMG_CHAIN", "2")
    try:
        pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
    finally:
        pm.set_merge_threshold(-1)
    _form(name, "chain form (P = 4)", "available" if op.chain_available() else "refused, patch form")
    ref = A.apply(u)
    if not op.chain_available():
        assert not op.chain_form()
        with pytest.raises(pm._lib.PmgError):
            op.set_chain_form(True)
        assert op.launches_per_apply() >= 3
        check_apply64(pm, name, op, layout, u, ref, what="apply fp64, chains refused", reps=3)
        return
    assert op.chain_form()
    check_apply64(pm, name, op, layout, u, ref, what="apply fp64, chain form", reps=3)
    check_apply32(name, op, u, A.apply(_f32(u)), lv.bc_marker, what="apply fp32, chain form on")
    op.set_chain_form(False)
    check_apply64(pm, name, op, layout, u, ref, what="apply fp64, chain form off", reps=1)


# ---------------------------------------------------------------------------------------------------------------------
# transfers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["coloured", "merged"])
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (1, 3), (3, 6), (4, 8), (2, 5)])
@pytest.mark.parametrize("name", ["star3", "star5 bent", "ogrid twisted"])
def test_transfers(pm, name, pc, pf, form):
    from oracle import pmg_oracle as po

    mesh = mesh_of(name, _size(pf))
    kappa = kappa_of(mesh.ncells)
    lc = mesh.level(pc)
    lf, Lf, fop = build_op(pm, mesh, pf, kappa, form)
    A = po.Laplacian(pf, kappa, lf.dofmap, mesh.xgeom, mesh.geom_dofmap, lf.bc_marker)
    oi = po.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lc.ndofs, lf.ndofs)
    Lc = pm.make_layout(lc)
    lcells, bcells = (lf.lcells, lf.bcells) if form == "coloured" else split_cells(mesh.ncells)
    rng = np.random.default_rng(pc * 10 + pf)
    uc, uf, zu = rng.standard_normal(lc.ndofs), rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)
    Puc, Ruf = oi.interpolate(uc), oi.reverse_interpolate(uf)
    fused_ref = oi.reverse_interpolate(uf - A.apply(zu))
    for tform, op_ in (("patch", fop), ("cell", None)):
        ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lcells, bcells, Lc, Lf, fine_operator=op_)
        vc, vf = _vec(pm, Lc, uc), pm.Vector(Lf)
        vf.set(4.0)
        ip.interpolate(vc, vf)
        got_p = vf.data_copy()
        _check(name, f"interpolate ({tform})", _relerr(got_p, Puc), TOL_PROLONG)
        vf2, vc2 = _vec(pm, Lf, uf), pm.Vector(Lc)
        for _ in range(2):
            vc2.set(3.0)
            ip.reverse_interpolate(vf2, vc2)
            _check(name, f"reverse_interpolate ({tform})", _relerr(vc2.data_copy(), Ruf), TOL)
        # <P u_c, u_f> = <u_c, P^T u_f> on what the device returned
        lhs, rhs = got_p @ uf, uc @ vc2.data_copy()
        _check(name, f"adjoint identity ({tform})", abs(lhs - rhs) / (np.abs(got_p) @ np.abs(uf)), TOL)
        z, coarse = _vec(pm, Lf, zu), pm.Vector(Lc)
        coarse.set(3.0)
        if op_ is None:
            with pytest.raises(pm._lib.PmgError):
                ip.restrict_residual(fop, z, vf2, coarse)
            continue
        vf3 = _vec(pm, Lf, uf)
        ip.interpolate_add(vc, vf3)
        _check(name, "interpolate_add", _relerr(vf3.data_copy(), uf + Puc), TOL_PROLONG)
        try:
            ip.restrict_residual(fop, z, vf2, coarse)
            available = True
        except pm._lib.PmgError:
            available = False
        _form(name, f"fused residual restriction ({pc}, {pf})", "available" if available else "refused, unfused sequence")
        if available:
            for _ in range(2):
                coarse.set(3.0)
                ip.restrict_residual(fop, z, vf2, coarse)
                _check(name, "restrict_residual", _relerr(coarse.data_copy(), fused_ref), TOL)
            assert np.array_equal(z.data_copy(), zu) and np.array_equal(vf2.data_copy(), uf)
        uc32, uf32, us32 = _f32(uc), _f32(uf), _f32(zu)
        fine = _dev32(uf32)
        ip.interpolate_add_fp32(_dev32(uc32), fine)
        _check(name, "interpolate_add fp32", _relerr(_host(fine), uf32 + oi.interpolate(uc32)), TOL_TRANSFER32)
        for sub, ref in ((None, oi.reverse_interpolate(uf32)), (_dev32(us32), oi.reverse_interpolate(uf32 - us32))):
            coarse32 = torch.full((lc.ndofs,), float("nan"), dtype=torch.float32, device="cuda")
            ip.reverse_interpolate_fp32(_dev32(uf32), coarse32, fine_sub=sub)
            _check(name, "reverse_interpolate fp32", _relerr(_host(coarse32), ref), TOL_TRANSFER32)
    _form(name, "patch-form transfer", "accepted")


# ---------------------------------------------------------------------------------------------------------------------
# cycles
# ---------------------------------------------------------------------------------------------------------------------

CYCLE_K = 3
CYCLES = [("star5 bent", (1, 2, 4)), ("ogrid twisted", (1, 2, 4)), ("star5 bent", (1, 3, 6)), ("ogrid twisted", (1, 3, 6))]
_ORACLE_CYCLES = {}


def oracle_cycle(name, orders):
    from oracle import pmg_oracle as po

    key = (name, orders)
    if key not in _ORACLE_CYCLES:
        mesh = mesh_of(name, "M" if orders[-1] == 4 else "S")
        _ORACLE_CYCLES[key] = (mesh,) + po.build_hierarchy(None, orders, cheb_its=CYCLE_K, mesh=mesh)[1:]
    return _ORACLE_CYCLES[key]


@pytest.mark.parametrize("name,orders", CYCLES)
def test_three_cycles_graph_replay_and_fp32_pcg(pm, name, orders):
    mesh, ops, sm, it, mg, b, eigs = oracle_cycle(name, orders)
    h = pm.PoissonHierarchy(None, orders, kappa=2.0, cheb_its=CYCLE_K, part=mesh)
    for got, ref in zip(h.eig_ranges, eigs):
        _check(name, "cycle: eigenvalue bound", abs(got[1] - ref[1]) / ref[1], TOL_EIG)
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    _check(name, "cycle: right-hand side", _relerr(h.rhs[-1].data_copy(), b), TOL)
    h.mg.set_graph(False)
    x = h.new_vector()
    x.set(0.0)
    xo = np.zeros_like(b)
    eager, first = [], None
    for _ in range(3):
        rn = h.mg.apply(h.rhs[-1], x, verbose=True)
        xo = mg.apply(b, xo, compute_rnorm=True)
        first = xo if first is None else first
        _check(name, "cycle: three V-cycles fp64", _relerr(x.data_copy(), xo), TOL_CYCLE)
        _check(name, "cycle: residual norm", abs(rn - mg.rnorm) / mg.rnorm, TOL_RNORM)
        eager.append((x.data_copy(), rn))
    assert eager[-1][1] < 0.5 * eager[0][1]  # the cycle contracts on such a mesh (the oracle's: 0.05 to 0.17)
    # replayed as a graph
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    x.set(0.0)
    for i in range(3):
        rn = h.mg.apply(h.rhs[-1], x, verbose=True)
        _check(name, "cycle: graph replay against eager", _relerr(x.data_copy(), eager[i][0]), TOL_GRAPH)
        assert abs(rn - eager[i][1]) < 1e-12 * eager[i][1]
    assert h.mg.graph_replays() == n0 + 3
    h.mg.set_graph(False)
    # the FP32 cycle against the oracle, then inside FP64 PCG
    h.mg.set_precision("fp32")
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)
    _check(name, "cycle: one V-cycle fp32", _relerr(x.data_copy(), first), TOL_CYCLE32)
    h.mg.set_precision("fp64")

    def pcg():
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(60)
        cg.set_tolerance(1e-8)
        xs = h.new_vector()
        xs.set(0.0)
        its = cg.solve(h.operators[-1], xs, h.rhs[-1], preconditioner=h.mg)
        r = pm.Vector(h.layouts[-1])
        h.operators[-1](xs, r)
        pm.axpy(r, -1.0, r, h.rhs[-1])
        return its, pm.norm(r) / pm.norm(h.rhs[-1])

    its64, res64 = pcg()
    h.mg.set_precision("fp32")
    its32, res32 = pcg()
    h.mg.set_precision("fp64")
    print(f"multiblock: {name} {orders}: PCG iterations fp64 cycle {its64}, fp32 cycle {its32}; residuals "
          f"{res64:.2e}, {res32:.2e}")
    assert abs(its32 - its64) <= 1 and its64 <= 25  # (the oracle's PCG: 11 to 17)
    assert res64 < 1e-7 and res32 < 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# the assembled operator
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("name", ["star5 bent", "ogrid twisted"])
def test_matrix_operator(pm, name, P):
    from oracle import pmg_oracle as po

    mesh = mesh_of(name, "S")
    kappa = kappa_of(mesh.ncells)
    lv, layout, op = build_op(pm, mesh, P, kappa, "merged")
    A = po.Laplacian(P, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.bc_marker)
    M = pm.MatrixOperator(op)
    ref, got = A.assemble_csr(), M.to_scipy()
    amax = np.abs(ref.data).max()
    dm = np.asarray(lv.dofmap, dtype=np.int64)
    pairs = np.unique(np.repeat(dm, dm.shape[1], axis=1).ravel() * lv.ndofs + np.tile(dm, (1, dm.shape[1])).ravel())
    assert got.shape == ref.shape and M.nnz == pairs.size  # every pair of dofs that shares a cell, valence 10 included
    diff = abs(got - ref)
    _check(name, "MatrixOperator entries", (diff.max() if diff.nnz else 0.0) / amax, TOL)
    sym = abs(got - got.T)
    assert (sym.max() if sym.nnz else 0.0) <= 1e-13 * amax
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(-3.0)
    M(x, y)
    _check(name, "MatrixOperator product", _relerr(y.data_copy(), A.apply(u)), TOL)
    d = pm.Vector(layout)
    M.get_diag_inverse(d)
    _check(name, "MatrixOperator diagonal", _relerr(d.data_copy(), A.diag_inverse()), TOL)


@pytest.mark.parametrize("name", ["star5 bent", "ogrid twisted"])
def test_cycle_with_an_assembled_level(pm, name):
    orders = (1, 2, 4)
    mesh, ops, sm, it, mg, b, eigs = oracle_cycle(name, orders)
    h = pm.PoissonHierarchy(None, orders, kappa=2.0, cheb_its=CYCLE_K, part=mesh, assembled_levels=(0,))
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)
    xo = mg.apply(b, np.zeros_like(b))
    _check(name, "cycle: one V-cycle, assembled level 0", _relerr(x.data_copy(), xo), TOL_CYCLE)


# ---------------------------------------------------------------------------------------------------------------------
# AMG at degree 1
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["star5 bent", "ogrid twisted"])
def test_amg(pm, name):
    """The checks of test_gpu_amg.py::test_hierarchy_against_first_principles and ::test_cycle_equals_numpy_restatement
    on a degree-1 graph whose vertices have 3 to 10 cells around them."""
    from oracle import pmg_oracle as po
    from oracle.amg_oracle import AmgCycle

    mesh = mesh_of(name, "L")
    lv = mesh.level(1)
    layout = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    op.compute_diag_inverse()
    k = 2
    amg = pm.AmgSolver(op, smoother_iterations=k)
    L = amg.num_levels()
    assert L >= 2 and amg.level_info(L - 1)["rows"] <= 800
    As = [amg.export(l, "A") for l in range(L)]
    Ps = [amg.export(l, "P") for l in range(L - 1)]
    ref = po.Laplacian(1, 2.0, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lv.bc_marker).assemble_csr()
    _check(name, "AMG: level 0 against the oracle's matrix", abs(As[0] - ref).max() / abs(ref).max(), TOL)
    bc = lv.bc_marker.astype(bool)
    for l in range(L - 1):
        G = (Ps[l].T @ As[l] @ Ps[l]).tocsr()
        _check(name, "AMG: Galerkin product", abs(G - As[l + 1]).max() / abs(As[l + 1]).max(), TOL)
        _check(name, "AMG: symmetry", abs(As[l + 1] - As[l + 1].T).max() / abs(As[l + 1]).max(), TOL)
        assert As[l + 1].shape[0] < 0.35 * As[l].shape[0]  # real coarsening
        if l == 0:
            assert abs(Ps[0][bc]).sum() == 0.0  # no Dirichlet row in P
            assert np.asarray((Ps[0] != 0).sum(axis=0)).ravel().min() >= 1
    assert np.linalg.eigvalsh(As[-1].toarray()).min() > 0
    info = amg.info()
    assert sum(i["nnz"] for i in info) / info[0]["nnz"] < 2.5  # operator complexity
    print(f"multiblock: {name}: AMG level sizes {[A.shape[0] for A in As]}")
    refc = AmgCycle(As, Ps, [amg.level_info(l)["lambda_max"] for l in range(L)], k)
    rng = np.random.default_rng(1)
    b = rng.standard_normal(lv.ndofs)
    b[bc] = 0.0
    x = pm.Vector(layout)
    x.set(7.0)
    amg.cycle(x, _vec(pm, layout, b))
    want = refc.cycle(b)
    _check(name, "AMG: cycle against the numpy restatement", np.abs(x.data_copy() - want).max() / np.abs(want).max(),
           TOL_AMG)
    c = rng.standard_normal(lv.ndofs)
    c[bc] = 0.0
    y = pm.Vector(layout)
    amg.cycle(y, _vec(pm, layout, c))
    assert abs(c @ x.data_copy() - b @ y.data_copy()) < 1e-10 * abs(c @ x.data_copy())
    amg2 = pm.AmgSolver(op, max_iter=60, rtol=1e-8, smoother_iterations=k)
    xs = pm.Vector(layout)
    its = amg2.solve(xs, _vec(pm, layout, b))
    xr, its_ref = refc.pcg(lambda v: As[0] @ v, b, 1e-8, 60)
    print(f"multiblock: {name}: AMG-PCG iterations {its}, numpy {its_ref}")
    assert its == its_ref and its <= 14
    _check(name, "AMG: PCG solution against numpy", np.abs(xs.data_copy() - xr).max() / np.abs(xr).max(), 1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# terms: one combined case per mesh
# ---------------------------------------------------------------------------------------------------------------------

def alpha_fun(pts):
    return 0.5 + (pts[:, 0] + 1.0) + 0.5 * (1.0 + pts[:, 1] * pts[:, 2]) ** 2


def h_fun(pts):
    return np.sin(2.0 * pts[:, 0]) + pts[:, 1] ** 2 - 0.7 * pts[:, 2]


def kq_fun(c):
    return 1.0 + 0.5 * np.sin(2.0 * c[:, 0] + c[:, 1]) * np.cos(c[:, 2])


def _low_side(mesh):
    """Dirichlet where x + y + z lies below the middle of its range: about half of the exterior, the rest natural."""
    s = mesh.xgeom.sum(axis=1)
    mid = 0.5 * (s.min() + s.max())
    return lambda c: c.sum(axis=1) < mid


@pytest.mark.parametrize("name", ["star5 bent", "ogrid twisted", "notched"])
def test_all_terms_combined(pm, name):
    """Nodal field, per-cell tensor, reaction and a Robin term on the mesh's own exterior facets (on the notched grid
    those of the cavity and of the notch among them): apply, diagonal, lifting, Neumann load and one V-cycle."""
    from oracle import pmg_oracle as po

    P, orders = 2, (1, 2)

    def fresh():  # (a hierarchy with ``dirichlet=`` narrows the markers of the mesh object it is given)
        return {"star5 bent": lambda: mb.star(5, 2, 2, bend=0.3), "ogrid twisted": lambda: mb.ogrid(2, map=twist),
                "notched": lambda: mb.notched((4, 3, 8))}[name]()

    mesh = fresh()
    keep = _low_side(mesh)
    cells, facets = mesh.exterior_facets()
    T = tc.random_spd(mesh.ncells, 5)
    sigma = rr.random_sigma(mesh.ncells, 6)
    kappa = 1.5

    def level(Pl):
        lv = mesh.level(Pl)
        coords = mesh.dof_coordinates(Pl)
        marker = (lv.bc_marker.astype(bool) & keep(coords)).astype(np.int8)
        assert 0 < marker.sum() < lv.bc_marker.sum()
        alpha = alpha_fun(mesh.facet_point_coordinates(Pl, cells, facets).reshape(-1, 3)).reshape(len(cells), -1)
        assert alpha.min() > 0
        A = tc.with_tensor(tc.laplacian(Pl, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, marker), T, kq_fun(coords))
        d_s = rr.reaction_vector(Pl, sigma, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, marker)
        d_r = rb.robin_vector(mesh, Pl, lv.dofmap, cells, facets, alpha, marker)
        return lv, coords, marker, alpha, A, d_s, d_r

    if name == "notched":
        # facets strictly inside the bounding box (the cavity, the notch) carry the Robin term
        pts = mesh.facet_point_coordinates(1, cells, facets).mean(axis=1)
        inside = ((pts > 1e-9) & (pts < 1 - 1e-9)).all(axis=1)
        assert inside.sum() >= 6 + 4
    lv, coords, marker, alpha, A, d_s, d_r = level(P)
    assert d_r.max() > 0 and d_s.max() > 0
    m = marker.astype(bool)
    layout = pm.make_layout(lv)
    lcells, bcells = split_cells(mesh.ncells)
    op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, lcells, bcells, marker, layout)
    op.set_coefficient_field(_vec(pm, layout, kq_fun(coords)))
    op.set_coefficient_tensor(T)
    op.set_reaction(sigma)
    op.set_robin(cells, facets, alpha)
    d = d_s + d_r
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    check_apply64(pm, name, op, layout, u, A.apply(u) + d * u, what="apply fp64, all terms")
    u32 = _f32(u)
    check_apply32(name, op, u, A.apply(u32) + d * u32, marker, what="apply fp32, all terms")
    op.compute_diag_inverse()
    dv = pm.Vector(layout)
    op.get_diag_inverse(dv)
    _check(name, "diag_inverse, all terms", _relerr(dv.data_copy(), 1.0 / (A.diagonal() + d)), TOL)
    # lifting of non-zero Dirichlet data, and the Neumann load of the same facets
    rng = np.random.default_rng(9)
    g = np.where(m, rng.standard_normal(lv.ndofs), np.nan)
    b0 = rng.standard_normal(lv.ndofs)
    nomark = np.zeros(lv.ndofs, dtype=np.int8)
    Afree = tc.with_tensor(tc.laplacian(P, kappa, lv.dofmap, mesh.xgeom, mesh.geom_dofmap, nomark), T, kq_fun(coords))
    want = np.where(m, b0, b0 - Afree.apply(np.where(m, g, 0.0)))
    bv = _vec(pm, layout, b0)
    op.apply_lifting(_vec(pm, layout, g), bv)
    got = bv.data_copy()
    assert not np.isnan(got).any() and np.array_equal(got[m], b0[m])
    _check(name, "apply_lifting, all terms", _relerr(got[~m], want[~m]), TOL)
    hq = h_fun(mesh.facet_point_coordinates(P, cells, facets).reshape(-1, 3)).reshape(len(cells), -1)
    bn = _vec(pm, layout, b0)
    op.assemble_neumann(cells, facets, hq, bn)
    wantn = bd.neumann_reference(mesh, P, lv.dofmap, cells, facets, hq, marker, lv.ndofs)
    assert np.abs(wantn).max() > 1e-3
    _check(name, "assemble_neumann", _relerr(bn.data_copy() - b0, wantn), TOL)
    # one V-cycle of the whole problem
    h = pm.PoissonHierarchy(None, orders, kappa=kappa, cheb_its=3, part=fresh(), kappa_field=kq_fun,
                            kappa_tensor=lambda centres: T, reaction=lambda centres: sigma, robin=alpha_fun,
                            dirichlet=keep)
    oops = []
    for Pl in orders:
        _, _, mk, _, Al, ds, dr = level(Pl)
        oops.append(rb.RobinLaplacian(Al, dr, ds))
    sm = [po.Chebyshev(e, 3) for e in h.eig_ranges]
    it = [po.Interpolator(orders[0], orders[1], oops[0].dofmap, oops[1].dofmap, oops[0].ndofs, oops[1].ndofs)]
    mgo = po.MultigridPreconditioner(oops, sm, it, oops[0].bc)
    b = h.rhs[-1].data_copy()
    ref = mgo.apply(b, np.zeros_like(b))
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)
    free = ~m
    _check(name, "cycle: one V-cycle, all terms", _relerr(x.data_copy()[free], ref[free]), TOL_CYCLE)


# ---------------------------------------------------------------------------------------------------------------------
# two ranks as threads: the star cut between sectors, the irregular edge on the interface
# ---------------------------------------------------------------------------------------------------------------------

def test_two_ranks_cut_between_sectors(pm):
    import threading

    from oracle import pmg_oracle as po
    from test_gpu_distributed import _ThreadComm, _ThreadWorld

    name, orders, world = "star5 bent", (1, 2, 4), 2
    mesh = mesh_of(name, "M")
    owner = mesh.cell_block * world // 5  # sectors 0, 1, 2 / 3, 4
    kappa = kappa_of(mesh.ncells)
    refs = {}
    for P in (2, 4):
        A = po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P))
        ug = np.random.default_rng(11).standard_normal(A.ndofs)
        refs[P] = (ug, A.apply(ug))
    _, ops, sm, it, mg, b, eigs = oracle_cycle(name, orders)
    W = _ThreadWorld(world)
    res, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                comm = _ThreadComm(W, rank)
                part = mesh.partition(owner, rank)
                out = {"apply": [], "ghosts": []}
                for P in (2, 4):
                    lv = part.level(P)
                    layout = pm.make_layout(lv, comm=comm)
                    op = pm.MatFreeLaplacian(P, kappa[part.cells], lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells,
                                             lv.bcells, lv.bc_marker, layout)
                    ug, want = refs[P]
                    xl = np.zeros(lv.ndofs)
                    xl[: lv.size_local] = ug[lv.local_to_global[: lv.size_local]]  # ghosts stale
                    x, y = _vec(pm, layout, xl), pm.Vector(layout)
                    op(x, y)
                    ref = want[lv.local_to_global[: lv.size_local]]
                    out["apply"].append(float(np.abs(y.data_copy()[: lv.size_local] - ref).max() / np.abs(want).max()))
                    out["ghosts"].append(bool(np.array_equal(x.data_copy(), ug[lv.local_to_global])))
                H = pm.PoissonHierarchy(None, orders, kappa=2.0, cheb_its=CYCLE_K, part=part, rank=rank, size=world,
                                        comm=comm)
                out["eig"] = H.eig_ranges
                W.wait()  # (rank 0 publishes the bounds the oracle's smoothers take)
                lvf = H.levels[-1]
                xv = H.new_vector()
                xv.set(0.0)
                out["iterates"], out["rnorm"] = [], []
                for _ in range(2):
                    out["rnorm"].append(H.mg.apply(H.rhs[-1], xv, verbose=True))
                    out["iterates"].append(xv.data_copy()[: lvf.size_local])
                out["l2g"] = lvf.local_to_global[: lvf.size_local]
                out["num_ghosts"] = [l.num_ghosts for l in H.levels]
                res[rank] = out
                torch.cuda.current_stream().synchronize()
        except BaseException:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            W.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, "\n".join(f"rank {r}:\n{tb}" for r, tb in errors)
    for out in res:
        assert all(out["ghosts"]) and all(g > 0 for g in out["num_ghosts"])
        _check(name, "two ranks: apply", max(out["apply"]), TOL)
        assert out["eig"] == res[0]["eig"]
    for got, ref in zip(res[0]["eig"], eigs):
        _check(name, "two ranks: eigenvalue bound", abs(got[1] - ref[1]) / ref[1], TOL_EIG)
    for s, e in zip(sm, res[0]["eig"]):
        s.eig_range = e
    xo = np.zeros_like(b)
    for i in range(2):
        xo = mg.apply(b, xo, compute_rnorm=True)
        for out in res:
            _check(name, "two ranks: V-cycle", np.abs(out["iterates"][i] - xo[out["l2g"]]).max() / np.abs(xo).max(),
                   TOL_CYCLE)
            assert abs(out["rnorm"][i] - mg.rnorm) < 1e-8 * mg.rnorm
