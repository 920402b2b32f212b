"""Every cell-indexed kernel on meshes whose cells carry arbitrary local frames (``BoxPartition(cell_frames=...)``): axes
permuted and reversed per cell, left-handed cells (det J < 0) included -- what a dolfinx or gmsh hexahedral mesh hands
the library.  Re-framing changes neither the global matrix, the load vectors, the transfer matrices nor the iterates, so
the reference is always the oracle (or a tests/*_reference.py module) on the FRAME-FREE mesh: other arrays, another
order of every cell's sums.  Bounds are those the existing test of the same quantity asserts against the oracle
(test_gpu_parity.py, test_gpu_fp32_kernels.py, test_gpu_boundary_data.py, test_gpu_matrix_operator.py,
test_gpu_distributed.py); the worst observed value of each family is printed (profiles/cell_frames.md)."""
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
import tensor_coefficient_reference as tc  # noqa: E402
from boundary_data_reference import twist, warp  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12  # FP64 apply, diagonal, load vectors, boundary terms, matrix entries (test_gpu_parity / _boundary_data)
TOL_G = 1e-13  # the exported tensor (test_gpu_parity.py::test_apply_parity_all_degrees)
TOL_PROLONG = 1e-13  # test_gpu_parity.py::test_transfer_parity
TOL_APPLY32 = 3e-6  # test_gpu_fp32_kernels.py: TOL_APPLY
TOL_TRANSFER32 = 2.5e-6  # ... TOL_TRANSFER
TOL_CYCLE32 = 1.8e-6  # ... TOL_CYCLE_ORACLE
TOL_CYCLE = 1e-10  # test_gpu_distributed.py: vcycle_err
TOL_CYCLE_AMG = 1e-7  # ... amg_vcycle_err
TOL_EIG = 1e-8

OBSERVED = {}


def _check(what, err, tol):
    OBSERVED[what] = max(OBSERVED.get(what, 0.0), float(err))
    print(f"cell frames: {what} {err:.3e} (worst so far {OBSERVED[what]:.3e}, bound {tol:.1e})")
    assert err < tol, (what, err, tol)


def shear(x):
    """Affine, not diagonal: every cell the same parallelepiped."""
    return x @ np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]]).T


def stretch(x):
    """Separable: the centroids stay on a tensor grid (tensor-block patches, two-stream halves)."""
    return x + 0.05 * np.sin(2.0 * np.pi * x)


MAPS = {"twist": twist, "warp": warp, "box": None, "shear": shear, "stretch": stretch}
N48 = (4, 3, 4)  # 48 cells: with "mixed" frames every symmetry occurs exactly once
N12 = (2, 2, 3)  # degrees 6 and 8
UNIFORM = {"cyclic": ((1, 2, 0), (0, 0, 0)), "swap": ((1, 0, 2), (0, 0, 0)), "flip": ((0, 1, 2), (0, 1, 0))}
FRAME_KINDS = ["mixed", "cyclic", "swap", "flip"]


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


def frames_for(pm, n, kind):
    """The frame table of a mesh: "mixed" is a fixed draw that holds both signs (on 48 cells a permutation of 0..47:
    every symmetry once); the uniform kinds give every cell the same non-identity symmetry."""
    syms = pm.cell_symmetries()
    ncells = int(np.prod(n))
    if kind == "mixed":
        rng = np.random.default_rng(ncells)
        fr = rng.permutation(48) if ncells == 48 else rng.integers(0, 48, ncells)
        signs = {syms[f][2] for f in fr}
        assert signs == {-1, 1}
        return fr.reshape(n)
    perm, flips = UNIFORM[kind]
    idx = [i for i, s in enumerate(syms) if s[0] == perm and s[1] == flips]
    assert len(idx) == 1 and idx[0] != 0
    return np.full(n, idx[0], dtype=np.int64)


_MESHES = {}


def mesh_pair(pm, n, wf, kind):
    """(frame-free partition, re-framed partition) of the same mesh, built once."""
    key = (tuple(n), wf, kind)
    if key not in _MESHES:
        _MESHES[key] = (pm.BoxPartition(n, warp=MAPS[wf]),
                        pm.BoxPartition(n, warp=MAPS[wf], cell_frames=frames_for(pm, n, kind)))
    return _MESHES[key]


def split_cells(ncells, seed=1):
    """Both cell lists non-empty (the library must not care which cell is in which)."""
    mask = np.random.default_rng(seed).uniform(size=ncells) < 0.7
    l, b = np.nonzero(mask)[0].astype(np.int32), np.nonzero(~mask)[0].astype(np.int32)
    assert l.size and b.size
    return l, b


def kappa_of(ncells):
    return np.random.default_rng(3).uniform(0.5, 3.0, ncells)


def build_op(pm, part, P, kappa, marker=None, split=True):
    lv = part.level(P)
    layout = pm.make_layout(lv)
    bc = lv.bc_marker if marker is None else np.ascontiguousarray(marker, dtype=np.int8)
    lcells, bcells = split_cells(part.ncells) if split else (lv.lcells, lv.bcells)
    op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lcells, bcells, bc, layout)
    return lv, layout, op


def check_apply64(pm, op, layout, u, ref, what="apply fp64", reps=2):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    for rep in range(reps):
        y.set(7.0 + rep)
        op(x, y)
        _check(what, _relerr(y.data_copy(), ref), TOL)


def check_apply32(op, u, ref32, bc, what="apply fp32"):
    x = _dev32(u)
    y = torch.full((x.numel(),), float("nan"), dtype=torch.float32, device="cuda")
    op.apply_fp32(x, y)
    got = _host(y)
    _check(what, _relerr(got, ref32), TOL_APPLY32)
    m = np.asarray(bc).astype(bool)
    assert np.array_equal(got[m], _f32(u[m]))


# ---------------------------------------------------------------------------------------------------------------------
# apply (FP64, FP32), inverse diagonal, load vector, exported tensor
# ---------------------------------------------------------------------------------------------------------------------

APPLY_CASES = ([(N48, wf, "mixed", P) for wf in ("twist", "warp") for P in (1, 2, 3, 4)]
               + [(N12, "twist", "mixed", P) for P in (6, 8)]
               + [(N48, "twist", kind, P) for kind in ("cyclic", "swap", "flip") for P in (1, 2, 3, 4)]
               + [(N12, "twist", kind, P) for kind in ("cyclic", "swap", "flip") for P in (6, 8)])


@pytest.mark.parametrize("n,wf,kind,P", APPLY_CASES)
def test_apply_diagonal_rhs_geometry(pm, n, wf, kind, P):
    from oracle import pmg_oracle as po

    p0, p1 = mesh_pair(pm, n, wf, kind)
    kappa = kappa_of(p0.ncells)
    l0 = p0.level(P)
    A = po.Laplacian(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    lv, layout, op = build_op(pm, p1, P, kappa)
    assert op.is_affine() == (wf == "warp")
    u = np.random.default_rng(10 + P).standard_normal(lv.ndofs)
    check_apply64(pm, op, layout, u, A.apply(u))
    check_apply32(op, u, A.apply(_f32(u)), lv.bc_marker)
    op.compute_diag_inverse()
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    _check("diag_inverse", _relerr(d.data_copy(), A.diag_inverse()), TOL)
    # load vector: f at the partition's own (re-framed) dof coordinates -- the same points, dof by dof
    c = p1.dof_coordinates(P)
    assert _relerr(c, p0.dof_coordinates(P)) < 1e-15
    fv = 29 * np.pi**2 * np.sin(2 * np.pi * c[:, 0]) * np.sin(3 * np.pi * c[:, 1]) * np.sin(4 * np.pi * c[:, 2])
    b = pm.Vector(layout)
    b.set(5.0)
    op.assemble_rhs(_vec(pm, layout, fv), b)
    _check("assemble_rhs", _relerr(b.data_copy(), A.rhs_manufactured(p0.dof_coordinates(P))), TOL)
    # the exported tensor, cell by cell: G'_{mn}(q') = s_m s_n G_{perm[m] perm[n]}(frame_node_map[q'])
    G = op.geometry().cpu().numpy()
    idx6 = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    syms = pm.cell_symmetries()
    want = np.empty_like(A.G)
    for cell in range(p0.ncells):
        perm, flips, _ = syms[p1.cell_frames[cell]]
        s = np.array([-1.0 if f else 1.0 for f in flips])
        old = A.G[cell][pm.frame_node_map(P, perm, flips)]  # [nq', 6] at the old node of every new node
        for k, (m, nn) in enumerate(tc.ORDER):
            want[cell, :, k] = s[m] * s[nn] * old[:, idx6[perm[m], perm[nn]]]
    _check("geometry()", _relerr(G, want), TOL_G)
    # a diagonal entry of G is positive whatever the frame: the sign of det J does not reach it
    assert (G[:, :, [0, 3, 5]] > 0).all()


# the smallest meshes of test_gpu_parity.py::test_two_stream_halves_agree_with_oracle
@pytest.mark.parametrize("kind", ["mixed", "cyclic"])
@pytest.mark.parametrize("P,n", [(1, (16, 8, 32)), (2, (16, 8, 32))])
def test_two_stream_halves(pm, P, n, kind, monkeypatch):
    from oracle import c_oracle as co

    p0, p1 = mesh_pair(pm, n, "stretch", kind)
    l0, lv = p0.level(P), p1.level(P)
    layout = pm.make_layout(lv)
    A = co.CLevel(P, 2.0, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    u = np.random.default_rng(11).standard_normal(lv.ndofs)
    monkeypatch.setenv("PMG_APPLY_STREAMS", "2")
    try:
        pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, p1.xgeom, p1.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
        ident = pm.MatFreeLaplacian(P, 2.0, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.lcells, l0.bcells, l0.bc_marker,
                                    layout)
    finally:
        pm.set_merge_threshold(-1)
    # the plan is made from centroids and dof sets: a frame does not change it
    assert ident.apply_streams() == 2
    assert op.apply_streams() == 2 and op.launches_per_apply() == ident.launches_per_apply()
    check_apply64(pm, op, layout, u, A.apply(u), what="apply fp64, two streams", reps=3)


# the smallest mesh of test_gpu_parity.py::test_chain_form_agrees_with_oracle that gets chains
@pytest.mark.parametrize("kind", ["cyclic", "swap", "flip", "mixed"])
def test_chain_form(pm, kind, monkeypatch):
    """Uniform non-identity frames keep the chain form; under mixed frames it is either correct or refused."""
    from oracle import c_oracle as co

    P, n = 4, (4, 4, 19)
    p0, p1 = mesh_pair(pm, n, "stretch", kind)
    l0, lv = p0.level(P), p1.level(P)
    layout = pm.make_layout(lv)
    A = co.CLevel(P, 2.0, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    u = np.random.default_rng(23).standard_normal(lv.ndofs)
    monkeypatch.setenv("PMG_CHAIN", "2")
    try:
        pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, p1.xgeom, p1.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
    finally:
        pm.set_merge_threshold(-1)
    if kind == "mixed" and not op.chain_available():
        with pytest.raises(pm._lib.PmgError):
            op.set_chain_form(True)
        check_apply64(pm, op, layout, u, A.apply(u), what="apply fp64, chains refused")
        return
    assert op.chain_available() and op.chain_form()
    assert op.launches_per_apply() <= 4
    ref = A.apply(u)
    check_apply64(pm, op, layout, u, ref, what="apply fp64, chain form", reps=3)
    check_apply32(op, u, A.apply(_f32(u)), lv.bc_marker, what="apply fp32, chain form on")
    op.set_chain_form(False)
    assert op.launches_per_apply() >= 8
    check_apply64(pm, op, layout, u, ref, what="apply fp64, chain form off", reps=1)


# ---------------------------------------------------------------------------------------------------------------------
# geometry modes
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", FRAME_KINDS)
@pytest.mark.parametrize("wf,P", [("box", 1), ("box", 2), ("box", 3), ("box", 4), ("shear", 2), ("shear", 4)])
def test_geometry_modes(pm, wf, P, kind):
    """Affine cells stay affine in every frame, reflected ones included; the constant-tensor apply and the batched
    geometry give the stored-tensor product."""
    from oracle import pmg_oracle as po
    from pmg_dolfinx_amd import _lib

    p0, p1 = mesh_pair(pm, N48, wf, kind)
    kappa = kappa_of(p0.ncells)
    l0 = p0.level(P)
    A = po.Laplacian(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    lv, layout, op = build_op(pm, p1, P, kappa)
    assert op.is_affine()
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    ref = A.apply(u)
    check_apply64(pm, op, layout, u, ref, what="apply fp64, stored", reps=1)
    op.set_geometry_mode("affine")
    check_apply64(pm, op, layout, u, ref, what="apply fp64, affine mode")
    check_apply32(op, u, A.apply(_f32(u)), lv.bc_marker, what="apply fp32, affine mode")
    op.set_geometry_mode("stored")
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 8)  # far fewer cells than the mesh: no resident tensor
    try:
        check_apply64(pm, op, layout, u, ref, what="apply fp64, batched geometry")
        op.compute_diag_inverse()
        d = pm.Vector(layout)
        op.get_diag_inverse(d)
        _check("diag_inverse, batched geometry", _relerr(d.data_copy(), A.diag_inverse()), TOL)
    finally:
        _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)


@pytest.mark.parametrize("P", [2, 3])
def test_batched_geometry_on_trilinear_cells(pm, P):
    from oracle import pmg_oracle as po
    from pmg_dolfinx_amd import _lib

    p0, p1 = mesh_pair(pm, N48, "twist", "mixed")
    kappa = kappa_of(p0.ncells)
    l0 = p0.level(P)
    A = po.Laplacian(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    lv, layout, op = build_op(pm, p1, P, kappa)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 8)
    try:
        check_apply64(pm, op, layout, u, A.apply(u), what="apply fp64, batched geometry")
    finally:
        _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)


# ---------------------------------------------------------------------------------------------------------------------
# transfers: the pairs of test_gpu_parity.py::test_irregular_numbering, the same frame table on both levels
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mixed", "swap"])
@pytest.mark.parametrize("pc,pf,n", [(1, 2, N48), (2, 4, N48), (3, 6, N12), (4, 8, N12)])
def test_transfers(pm, pc, pf, n, kind):
    from oracle import pmg_oracle as po

    p0, p1 = mesh_pair(pm, n, "twist", kind)
    kappa = kappa_of(p0.ncells)
    c0, f0 = p0.level(pc), p0.level(pf)
    lc, lf = p1.level(pc), p1.level(pf)
    A = po.Laplacian(pf, kappa, f0.dofmap, p0.xgeom, p0.geom_dofmap, f0.bc_marker)
    oi = po.Interpolator(pc, pf, c0.dofmap, f0.dofmap, c0.ndofs, f0.ndofs)
    Lc = pm.make_layout(lc)
    _, Lf, fop = build_op(pm, p1, pf, kappa)
    lcells, bcells = split_cells(p1.ncells)
    rng = np.random.default_rng(pc * 10 + pf)
    uc, uf, zu = rng.standard_normal(lc.ndofs), rng.standard_normal(lf.ndofs), rng.standard_normal(lf.ndofs)
    Puc, Ruf = oi.interpolate(uc), oi.reverse_interpolate(uf)
    fused_ref = oi.reverse_interpolate(uf - A.apply(zu))
    for form, op_ in (("patch", fop), ("cell", None)):
        ip = pm.Interpolator(pc, pf, lc.dofmap, lf.dofmap, lcells, bcells, Lc, Lf, fine_operator=op_)
        vc, vf = _vec(pm, Lc, uc), pm.Vector(Lf)
        vf.set(4.0)
        ip.interpolate(vc, vf)
        _check(f"interpolate ({form})", _relerr(vf.data_copy(), Puc), TOL_PROLONG)
        vf2, vc2 = _vec(pm, Lf, uf), pm.Vector(Lc)
        for _ in range(2):
            vc2.set(3.0)
            ip.reverse_interpolate(vf2, vc2)
            _check(f"reverse_interpolate ({form})", _relerr(vc2.data_copy(), Ruf), TOL)
        z, coarse = _vec(pm, Lf, zu), pm.Vector(Lc)
        coarse.set(3.0)
        if op_ is None:
            # no fine operator: the library has no fused form (an error code, nothing written)
            with pytest.raises(pm._lib.PmgError):
                ip.restrict_residual(fop, z, vf2, coarse)
            with pytest.raises(RuntimeError):
                ip.interpolate_add(vc, pm.Vector(Lf))
            continue
        vf3 = _vec(pm, Lf, uf)
        ip.interpolate_add(vc, vf3)
        _check("interpolate_add", _relerr(vf3.data_copy(), uf + Puc), TOL_PROLONG)
        # fused residual restriction: available for the same pairs as on the frame-free mesh, and then the oracle's
        l0cells, b0cells = split_cells(p0.ncells)
        fop0 = pm.MatFreeLaplacian(pf, kappa, f0.dofmap, p0.xgeom, p0.geom_dofmap, l0cells, b0cells, f0.bc_marker, Lf)
        ip0 = pm.Interpolator(pc, pf, c0.dofmap, f0.dofmap, l0cells, b0cells, Lc, Lf, fine_operator=fop0)
        try:
            ip0.restrict_residual(fop0, z, vf2, coarse)
            available = True
        except pm._lib.PmgError:
            available = False
        if available:
            for _ in range(2):
                coarse.set(3.0)
                ip.restrict_residual(fop, z, vf2, coarse)
                _check("restrict_residual", _relerr(coarse.data_copy(), fused_ref), TOL)
            assert np.array_equal(z.data_copy(), zu) and np.array_equal(vf2.data_copy(), uf)
        else:
            with pytest.raises(pm._lib.PmgError):
                ip.restrict_residual(fop, z, vf2, coarse)
        # FP32 forms, against the FP64 oracle on the float-rounded inputs
        uc32, uf32, us32 = _f32(uc), _f32(uf), _f32(zu)
        fine = _dev32(uf32)
        ip.interpolate_add_fp32(_dev32(uc32), fine)
        _check("interpolate_add fp32", _relerr(_host(fine), uf32 + oi.interpolate(uc32)), TOL_TRANSFER32)
        for sub, ref in ((None, oi.reverse_interpolate(uf32)), (_dev32(us32), oi.reverse_interpolate(uf32 - us32))):
            coarse32 = torch.full((lc.ndofs,), float("nan"), dtype=torch.float32, device="cuda")
            ip.reverse_interpolate_fp32(_dev32(uf32), coarse32, fine_sub=sub)
            _check("reverse_interpolate fp32", _relerr(_host(coarse32), ref), TOL_TRANSFER32)


# ---------------------------------------------------------------------------------------------------------------------
# terms: coefficient field, coefficient tensor, reaction, Robin, Neumann, lifting, set_bc
# ---------------------------------------------------------------------------------------------------------------------

def alpha_fun(pts):
    return 0.5 + pts[:, 0] + 2.0 * pts[:, 1] * pts[:, 2]


def h_fun(pts):
    return np.sin(2.0 * pts[:, 0]) + pts[:, 1] ** 2 - 0.7 * pts[:, 2]


def kq_fun(c):
    return 1.0 + 0.5 * np.sin(2.0 * c[:, 0] + c[:, 1]) * np.cos(c[:, 2])


class Terms:
    """One level of the 48-cell twisted mesh with mixed frames, Dirichlet on x = 0 only, and everything the frame-free
    references need."""

    def __init__(self, pm, P, kind="mixed"):
        self.pm, self.P = pm, P
        self.p0, self.p1 = mesh_pair(pm, N48, "twist", kind)
        p0, p1 = self.p0, self.p1
        self.l0 = p0.level(P)
        self.coords = p0.dof_coordinates(P)
        self.marker = rb.one_face_marker(self.l0.bc_marker, self.coords)
        assert 0 < self.marker.sum() < self.l0.bc_marker.sum()
        self.kappa = kappa_of(p0.ncells)
        self.lv, self.layout, self.op = build_op(pm, p1, P, self.kappa, marker=self.marker)
        self.nomark = np.zeros(self.l0.ndofs, dtype=np.int8)
        # facets: each partition's own list; coefficients as functions of each list's own facet points
        self.c0, self.f0 = p0.exterior_facets()
        self.c1, self.f1 = p1.exterior_facets()
        assert not np.array_equal(self.f0, self.f1)
        nf = (P + 1) ** 2
        self.pts0 = p0.facet_point_coordinates(P, self.c0, self.f0).reshape(-1, 3)
        self.pts1 = p1.facet_point_coordinates(P, self.c1, self.f1).reshape(-1, 3)
        self.alpha0, self.alpha1 = alpha_fun(self.pts0).reshape(-1, nf), alpha_fun(self.pts1).reshape(-1, nf)
        self.h0, self.h1 = h_fun(self.pts0).reshape(-1, nf), h_fun(self.pts1).reshape(-1, nf)
        centres = tc.cell_centres(p0.xgeom, p0.geom_dofmap)
        assert _relerr(tc.cell_centres(p1.xgeom, p1.geom_dofmap), centres) < 1e-15
        self.T = tc.random_spd(p0.ncells, 5)
        self.sigma = rr.random_sigma(p0.ncells, 6)
        self.kq = kq_fun(self.coords)
        self.u = np.random.default_rng(P).standard_normal(self.l0.ndofs)

    def oracle(self, marker=None):
        m = self.marker if marker is None else marker
        return tc.laplacian(self.P, self.kappa, self.l0.dofmap, self.p0.xgeom, self.p0.geom_dofmap, m)

    def check(self, A, what, d=None):
        """apply (FP64, FP32) and inverse diagonal of ``self.op`` against the oracle operator A plus the diagonal d."""
        pm, u = self.pm, self.u
        d = np.zeros(self.l0.ndofs) if d is None else d
        check_apply64(pm, self.op, self.layout, u, A.apply(u) + d * u, what=f"apply fp64, {what}")
        u32 = _f32(u)
        check_apply32(self.op, u, A.apply(u32) + d * u32, self.marker, what=f"apply fp32, {what}")
        self.op.compute_diag_inverse()
        dv = pm.Vector(self.layout)
        self.op.get_diag_inverse(dv)
        _check(f"diag_inverse, {what}", _relerr(dv.data_copy(), 1.0 / (A.diagonal() + d)), TOL)


@pytest.fixture(scope="module", params=[2, 3])
def terms(pm, request):
    return Terms(pm, request.param)


def test_coefficient_field_and_tensor(pm, terms):
    t = terms
    t.op.set_coefficient_field(_vec(pm, t.layout, t.kq))
    A = t.oracle()
    A.G = A.G * t.kq[A.dofmap][:, :, None]
    t.check(A, "coefficient field")
    t.op.set_coefficient_tensor(t.T)
    t.check(tc.with_tensor(t.oracle(), t.T, t.kq), "field and tensor")
    t.op.set_coefficient_field(None)
    t.check(tc.with_tensor(t.oracle(), t.T), "coefficient tensor")
    t.op.set_coefficient_tensor(None)
    t.check(t.oracle(), "terms removed")


def test_reaction(pm, terms):
    t = terms
    t.op.set_reaction(t.sigma)
    d = rr.reaction_vector(t.P, t.sigma, t.l0.dofmap, t.p0.xgeom, t.p0.geom_dofmap, t.marker)
    assert d.max() > 0
    t.check(t.oracle(), "reaction", d)
    t.op.set_reaction(None)


def test_robin_and_neumann(pm, terms):
    """New-frame facet numbers; alpha and h are functions of the new-frame facet-point coordinates."""
    t = terms
    t.op.set_robin(t.c1, t.f1, t.alpha1)
    d = rb.robin_vector(t.p0, t.P, t.l0.dofmap, t.c0, t.f0, t.alpha0, t.marker)
    assert d.max() > 0
    t.check(t.oracle(), "Robin", d)
    t.op.set_robin(None, None, None)
    b0 = np.random.default_rng(4).standard_normal(t.l0.ndofs)
    b = _vec(pm, t.layout, b0)
    t.op.assemble_neumann(t.c1, t.f1, t.h1, b)
    want = bd.neumann_reference(t.p0, t.P, t.l0.dofmap, t.c0, t.f0, t.h0, t.marker, t.l0.ndofs)
    assert np.abs(want).max() > 1e-3
    _check("assemble_neumann", _relerr(b.data_copy() - b0, want), TOL)
    # unit flux: the area of the twisted box's faces, frame by frame the same sum
    b.set(0.0)
    t.op.assemble_neumann(t.c1, t.f1, np.ones_like(t.h1), b)
    one = bd.neumann_reference(t.p0, t.P, t.l0.dofmap, t.c0, t.f0, np.ones_like(t.h0), t.marker, t.l0.ndofs)
    _check("assemble_neumann", _relerr(b.data_copy(), one), TOL)


def test_lifting_and_set_bc(pm, terms):
    t = terms
    m = t.marker.astype(bool)
    rng = np.random.default_rng(8)
    g = np.where(m, rng.standard_normal(t.l0.ndofs), np.nan)
    x0 = np.where(m, rng.standard_normal(t.l0.ndofs), np.nan)
    b0 = rng.standard_normal(t.l0.ndofs)
    Afree = t.oracle(t.nomark)
    for x0_, alpha in ((x0, 0.75), (None, 1.0)):
        lift = Afree.apply(np.where(m, g - (x0_ if x0_ is not None else 0.0), 0.0))
        want = np.where(m, b0, b0 - alpha * lift)
        bv = _vec(pm, t.layout, b0)
        t.op.apply_lifting(_vec(pm, t.layout, g), bv, x0=_vec(pm, t.layout, x0_) if x0_ is not None else None,
                           alpha=alpha)
        got = bv.data_copy()
        assert not np.isnan(got).any() and np.array_equal(got[m], b0[m])
        assert _relerr(want[~m], b0[~m]) > 1e-3
        _check("apply_lifting", _relerr(got[~m], want[~m]), TOL)
        t.op.set_bc(_vec(pm, t.layout, g), bv, x0=_vec(pm, t.layout, x0_) if x0_ is not None else None, alpha=alpha)
        got2 = bv.data_copy()
        assert np.array_equal(got2[~m], got[~m])
        assert np.array_equal(got2[m], alpha * ((g - x0_)[m] if x0_ is not None else g[m]))


def test_all_terms_combined(pm, terms):
    t = terms
    m = t.marker.astype(bool)
    t.op.set_coefficient_field(_vec(pm, t.layout, t.kq))
    t.op.set_coefficient_tensor(t.T)
    t.op.set_reaction(t.sigma)
    t.op.set_robin(t.c1, t.f1, t.alpha1)
    try:
        d = (rr.reaction_vector(t.P, t.sigma, t.l0.dofmap, t.p0.xgeom, t.p0.geom_dofmap, t.marker)
             + rb.robin_vector(t.p0, t.P, t.l0.dofmap, t.c0, t.f0, t.alpha0, t.marker))
        t.check(tc.with_tensor(t.oracle(), t.T, t.kq), "all terms", d)
        # the lifting follows the field and the tensor (the diagonal terms have no off-diagonal entry to lift)
        rng = np.random.default_rng(9)
        g = np.where(m, rng.standard_normal(t.l0.ndofs), np.nan)
        b0 = rng.standard_normal(t.l0.ndofs)
        Afree = tc.with_tensor(t.oracle(t.nomark), t.T, t.kq)
        want = np.where(m, b0, b0 - Afree.apply(np.where(m, g, 0.0)))
        bv = _vec(pm, t.layout, b0)
        t.op.apply_lifting(_vec(pm, t.layout, g), bv)
        _check("apply_lifting, all terms", _relerr(bv.data_copy()[~m], want[~m]), TOL)
        # the assembled operator of the same state
        M = pm.MatrixOperator(t.op)
        ref = (tc.with_tensor(t.oracle(), t.T, t.kq).assemble_csr()).tocsr()
        import scipy.sparse as sp

        ref = (ref + sp.diags(d)).tocsr()
        diff = abs(M.to_scipy() - ref)
        _check("MatrixOperator entries, all terms", (diff.max() if diff.nnz else 0.0) / np.abs(ref.data).max(), TOL)
    finally:
        t.op.set_robin(None, None, None)
        t.op.set_reaction(None)
        t.op.set_coefficient_tensor(None)
        t.op.set_coefficient_field(None)


# ---------------------------------------------------------------------------------------------------------------------
# the assembled operator
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mixed", "flip"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_matrix_operator(pm, P, kind):
    from oracle import pmg_oracle as po

    p0, p1 = mesh_pair(pm, N48, "twist", kind)
    kappa = kappa_of(p0.ncells)
    l0 = p0.level(P)
    A = po.Laplacian(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    lv, layout, op = build_op(pm, p1, P, kappa)
    M = pm.MatrixOperator(op)
    ref, got = A.assemble_csr(), M.to_scipy()
    amax = np.abs(ref.data).max()
    # dolfinx's pattern: every pair of dofs that shares a cell
    dm = np.asarray(l0.dofmap, dtype=np.int64)
    pairs = np.unique(np.repeat(dm, dm.shape[1], axis=1).ravel() * lv.ndofs + np.tile(dm, (1, dm.shape[1])).ravel())
    assert got.shape == ref.shape and M.nnz == pairs.size
    diff = abs(got - ref)
    _check("MatrixOperator entries", (diff.max() if diff.nnz else 0.0) / amax, TOL)
    sym = abs(got - got.T)
    assert (sym.max() if sym.nnz else 0.0) <= 1e-13 * amax
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    y.set(-3.0)
    M(x, y)
    _check("MatrixOperator product", _relerr(y.data_copy(), A.apply(u)), TOL)
    d = pm.Vector(layout)
    M.get_diag_inverse(d)
    _check("MatrixOperator diagonal", _relerr(d.data_copy(), A.diag_inverse()), TOL)


# ---------------------------------------------------------------------------------------------------------------------
# the cycle
# ---------------------------------------------------------------------------------------------------------------------

CYCLE_N, CYCLE_ORDERS, CYCLE_K = (6, 6, 6), (1, 2, 4), 3


@pytest.fixture(scope="module")
def cycle_oracle():
    from oracle import pmg_oracle as po

    return po.build_hierarchy(CYCLE_N, CYCLE_ORDERS, cheb_its=CYCLE_K, warp=warp)


def _cycle_frames(pm):
    fr = np.random.default_rng(216).integers(0, 48, CYCLE_N)
    assert {pm.cell_symmetries()[f][2] for f in fr.ravel()} == {-1, 1}
    return fr


def test_cycle_eigenvalues_and_two_cycles(pm, cycle_oracle):
    from oracle import pmg_oracle as po

    mesh, ops, sm, it, mg, b, eigs = cycle_oracle
    h = pm.PoissonHierarchy(CYCLE_N, CYCLE_ORDERS, kappa=2.0, cheb_its=CYCLE_K, warp=warp,
                            cell_frames=_cycle_frames(pm))
    for got, ref in zip(h.eig_ranges, eigs):
        _check("cycle: eigenvalue bound", abs(got[1] - ref[1]) / ref[1], TOL_EIG)
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    _check("cycle: right-hand side", _relerr(h.rhs[-1].data_copy(), b), TOL)

    def two_cycles(what, tol, mgo=mg):
        x = h.new_vector()
        x.set(0.0)
        xo = np.zeros_like(b)
        for _ in range(2):
            rn = h.mg.apply(h.rhs[-1], x, verbose=(tol == TOL_CYCLE))
            xo = mgo.apply(b, xo, compute_rnorm=True)
            _check(what, _relerr(x.data_copy(), xo), tol)
            if tol == TOL_CYCLE:
                assert abs(rn - mgo.rnorm) < 1e-8 * mgo.rnorm

    two_cycles("cycle: two V-cycles fp64", TOL_CYCLE)
    h.mg.set_precision("fp32")
    two_cycles("cycle: two V-cycles fp32", TOL_CYCLE32)
    h.mg.set_precision("fp64")
    # the AMG coarse solver against the oracle's cycle with an exact coarse solve (test_gpu_distributed.py)
    import scipy.sparse.linalg as spla

    lu = spla.splu(ops[0].assemble_csr().tocsc())

    def exact(u0, b0):
        u0[:] = lu.solve(b0)

    mgo = po.MultigridPreconditioner(ops, sm, it, mesh.boundary_marker(CYCLE_ORDERS[0]), coarse_solver=exact)
    h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0], max_iter=100, rtol=1e-11))
    two_cycles("cycle: two V-cycles, AMG coarse solver", TOL_CYCLE_AMG, mgo)
    h.mg.set_coarse_solver(None)
    # PCG: as many iterations as the frame-free hierarchy on the device
    h0 = pm.PoissonHierarchy(CYCLE_N, CYCLE_ORDERS, kappa=2.0, cheb_its=CYCLE_K, warp=warp)
    its = []
    for hh in (h, h0):
        cg = pm.CGSolver(hh.layouts[-1])
        cg.set_max_iterations(50)
        cg.set_tolerance(1e-8)
        x = hh.new_vector()
        x.set(0.0)
        its.append((cg.solve(hh.operators[-1], x, hh.rhs[-1], preconditioner=hh.mg), x.data_copy()))
    print(f"cell frames: PCG iterations with frames {its[0][0]}, frame-free {its[1][0]}")
    assert its[0][0] == its[1][0] and its[0][0] < 15
    _check("cycle: PCG solution against the frame-free device solve", _relerr(its[0][1], its[1][1]), 1e-8)


def test_cycle_with_an_assembled_level(pm, cycle_oracle):
    mesh, ops, sm, it, mg, b, eigs = cycle_oracle
    h = pm.PoissonHierarchy(CYCLE_N, CYCLE_ORDERS, kappa=2.0, cheb_its=CYCLE_K, warp=warp,
                            cell_frames=_cycle_frames(pm), assembled_levels=(0,))
    for s, e in zip(sm, h.eig_ranges):
        s.eig_range = e
    x = h.new_vector()
    x.set(0.0)
    xo = np.zeros_like(b)
    for _ in range(2):
        h.mg.apply(h.rhs[-1], x)
        xo = mg.apply(b, xo)
        _check("cycle: two V-cycles, assembled level 0", _relerr(x.data_copy(), xo), TOL_CYCLE)


# ---------------------------------------------------------------------------------------------------------------------
# two ranks: ghost cells whose frames differ from their owners' neighbours (plain exchange route)
# ---------------------------------------------------------------------------------------------------------------------

def test_two_ranks_with_cell_frames(pm):
    from test_gpu_distributed import _assert_rank_results, _run_ranks, _worker

    n, dims, orders = (3, 4, 8), (1, 1, 2), (1, 2, 4)
    frames = np.random.default_rng(96).integers(0, 48, n)
    res = _run_ranks(_worker, 2, (n, dims, orders, "exchange", frames))
    _assert_rank_results(res)
    for out in res:
        print(f"cell frames, two ranks: apply {max(out['apply_err']):.3e}, V-cycle "
              f"{max(e for e, _ in out['vcycle_err']):.3e}, AMG V-cycle {max(out['amg_vcycle_err']):.3e}")
