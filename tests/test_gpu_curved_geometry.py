"""Curved cells on the GPU: operators with a coordinate element of degree g = 2 ... 4 (``pmg_laplacian_create_curved``)
against tests/curved_geometry_reference.py -- the exported tensor by both geometry paths (the cell-cooperative kernel
for the library's own tabulation, the per-point one for caller tables), and every route that reaches the geometry:
coefficient field and tensor, batched geometry, affine mode, apply (FP64, FP32), diagonal, load vector, reaction, Neumann
and Robin terms on curved faces, lifting, the assembled matrix, the V-cycle, AMG and two ranks.

Meshes are the smallest that still hold several patches (tests/test_gpu_multiblock.py): a box of (6, 6, 16) cells at
P <= 2, (3, 4, 6) at P = 3, 4 and (2, 3, 3) above, mapped onto the quarter annulus, cells in frames drawn from all 48.
Bounds are the existing tests' for the same quantity; the worst value of each check is printed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import curved_geometry_reference as cg  # noqa: E402
from boundary_data_reference import twist  # noqa: E402
from tensor_coefficient_reference import random_spd  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12  # FP64 apply, diagonal, load vectors, boundary terms, matrix entries (test_gpu_parity / _boundary_data)
TOL_G = 1e-13  # the exported tensor, relative to max |G| (test_gpu_parity.py::test_apply_parity_all_degrees)
TOL_APPLY32 = 3e-6  # test_gpu_fp32_kernels.py: TOL_APPLY
TOL_CYCLE = 1e-10  # test_gpu_parity.py::test_vcycle_parity
TOL_AMG = 1e-11  # test_gpu_amg.py::test_cycle_equals_numpy_restatement
TOL_GRAPH = 1e-13  # test_gpu_parity.py::test_vcycle_graph_replay

OBSERVED = {}


def _check(what, err, tol):
    OBSERVED[what] = max(OBSERVED.get(what, 0.0), float(err))
    print(f"curved geometry: {what} {err:.3e} (worst so far {OBSERVED[what]:.3e}, bound {tol:.1e})")
    assert err < tol, (what, err, tol)


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


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _n(P):
    return (6, 6, 16) if P <= 2 else ((3, 4, 6) if P <= 4 else (2, 3, 3))


def kappa_of(ncells):
    return np.random.default_rng(3).uniform(0.5, 3.0, ncells)


def split_cells(ncells, seed=1):
    mask = np.random.default_rng(seed).uniform(size=ncells) < 0.7
    return np.nonzero(mask)[0].astype(np.int32), np.nonzero(~mask)[0].astype(np.int32)


_MESHES = {}


def mesh_pair(pm, n, g, warp=cg.quarter_annulus):
    """(frame-free partition, the same mesh with every cell in a frame drawn from all 48), built once."""
    key = (tuple(n), g, warp)
    if key not in _MESHES:
        fr = np.random.default_rng(int(np.prod(n)) + g).integers(0, 48, n)
        assert {pm.cell_symmetries()[f][2] for f in fr.ravel()} == {-1, 1}  # left-handed cells included
        _MESHES[key] = (pm.BoxPartition(n, warp=warp, geom_degree=g),
                        pm.BoxPartition(n, warp=warp, geom_degree=g, cell_frames=fr))
    return _MESHES[key]


def reference(p0, P, kappa, marker=None):
    l0 = p0.level(P)
    return cg.laplacian(P, p0.geom_degree, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap,
                        l0.bc_marker if marker is None else marker)


def build_op(pm, part, P, kappa, marker=None, form="merged", **kw):
    """form "coloured": one cell list, every colour a launch of its own; "merged": two cell lists, the default
    threshold (levels as small as these are merged)."""
    lv = part.level(P)
    layout = pm.make_layout(lv)
    bc = lv.bc_marker if marker is None else np.ascontiguousarray(marker, dtype=np.int8)
    lcells, bcells = (lv.lcells, lv.bcells) if form == "coloured" else split_cells(part.ncells)
    try:
        if form == "coloured":
            pm.set_merge_threshold(0)
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lcells, bcells, bc, layout,
                                 geometry_degree=part.geom_degree, **kw)
    finally:
        pm.set_merge_threshold(-1)
    assert op.geometry_degree() == part.geom_degree
    return lv, layout, op


IDX6 = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def framed(pm, part, P, G):
    """The frame-free tensor [ncells, nq, 6] as the re-framed partition's operator exports it:
    G'_{mn}(q') = s_m s_n G_{perm[m] perm[n]}(frame_node_map[q'])."""
    syms = pm.cell_symmetries()
    want = np.empty_like(G)
    for cell in range(part.ncells):
        perm, flips, _ = syms[part.cell_frames[cell]]
        s = np.array([-1.0 if f else 1.0 for f in flips])
        old = G[cell][pm.frame_node_map(P, perm, flips)]
        for k, (m, nn) in enumerate(cg.ORDER):
            want[cell, :, k] = s[m] * s[nn] * old[:, IDX6[perm[m], perm[nn]]]
    return want


def check_apply64(pm, op, layout, u, ref, what, reps=2):
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    for rep in range(reps):
        y.set(7.0 + rep)
        op(x, y)
        _check(what, _relerr(y.data_copy(), ref), TOL)


def check_apply32(op, u, ref32, bc, what):
    x = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()
    y = torch.full((x.numel(),), float("nan"), dtype=torch.float32, device="cuda")
    op.apply_fp32(x, y)
    torch.cuda.synchronize()
    got = y.cpu().numpy().astype(np.float64)
    _check(what, _relerr(got, ref32), TOL_APPLY32)
    m = np.asarray(bc).astype(bool)
    assert np.array_equal(got[m], _f32(u[m]))


def kq_fun(c):
    return 1.0 + 0.5 * np.sin(2.0 * c[:, 0] + c[:, 1]) * np.cos(c[:, 2])


def h_fun(pts):
    return np.sin(2.0 * pts[:, 0]) + pts[:, 1] ** 2 - 0.7 * pts[:, 2]


def alpha_fun(pts):
    return 0.5 + pts[:, 0] + 2.0 * pts[:, 1] * pts[:, 2]


# ---------------------------------------------------------------------------------------------------------------------
# 1. degree 1 through the new entry point: the bits of pmg_laplacian_create_ordered
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,n", [(2, (6, 6, 16)), (4, (3, 4, 6)), (2, (1, 1, 600)), (4, (1, 1, 72))])
def test_degree_one_is_bit_identical_to_the_old_entry_point(pm, P, n):
    """The exported tensor is compared bit for bit on the boxes of this file.  An apply, the diagonal and the load
    vector sum the cells around a dof with atomics, in no fixed order: on those boxes one and the same operator
    applied twice differs from itself in the last bit (measured: 232 of 5577 entries at P = 2, 53 of 5525 at P = 4,
    at most 7e-17 of max |y|; the diagonal and the load vector likewise), so a comparison of bits says nothing there.
    On a column of cells every dof lies in at most two cells and a two-term sum does not depend on its order (measured:
    0 differing entries, same operator twice and two operators): there all four are compared bit for bit, on meshes of
    several patches (600 cells at P = 2, 72 at P = 4)."""
    import ctypes as C

    from pmg_dolfinx_amd import _lib

    column = n[0] == 1
    part = pm.BoxPartition(n, warp=twist, cell_frames=np.random.default_rng(P).integers(0, 48, n))
    kappa = kappa_of(part.ncells)
    lv, layout, new = build_op(pm, part, P, kappa, form="coloured")
    lc, bc_ = lv.lcells, lv.bcells
    h = _lib.vp()
    pm.set_merge_threshold(0)
    _lib.call("pmg_laplacian_create_ordered", C.byref(h), layout.handle, P, part.ncells, _lib.ptr(new.kappa),
              _lib.ptr(new.dofmap), _lib.ptr(new.xgeom), int(new.xgeom.numel() // 3), _lib.ptr(new.geom_dofmap), None,
              None, lc.ctypes.data_as(_lib.c_ip), lc.size, bc_.ctypes.data_as(_lib.c_ip), bc_.size,
              _lib.ptr(new.bc_marker), 0, None, _lib.current_stream())
    pm.set_merge_threshold(-1)
    old = object.__new__(pm.MatFreeLaplacian)
    old.__dict__.update(new.__dict__)
    old._handle = h
    assert old.geometry_degree() == 1 and new.geometry_degree() == 1
    assert torch.equal(old.geometry(), new.geometry())
    assert old.is_affine() == new.is_affine() and old.launches_per_apply() == new.launches_per_apply()
    if not column:
        return
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    fv = np.random.default_rng(P + 1).standard_normal(lv.ndofs)
    outs = []
    for op in (old, new):
        x, y, b, d = _vec(pm, layout, u), pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
        op(x, y)
        op.compute_diag_inverse()
        op.get_diag_inverse(d)
        op.assemble_rhs(_vec(pm, layout, fv), b)
        outs.append((y.data_copy(), d.data_copy(), b.data_copy()))
    for name, a, b in zip(("apply", "inverse diagonal", "load vector"), outs[0], outs[1]):
        assert np.array_equal(a, b), name


# ---------------------------------------------------------------------------------------------------------------------
# 2. the exported tensor
# ---------------------------------------------------------------------------------------------------------------------

# (every case holds TOL_G: the worst is 3.5e-14 at P = 1, g = 3; the CPU's own spread between the two orders of the
# sum reaches 5.1e-14 at P = 8, g = 4 -- tests/test_curved_geometry_reference.py, profiles/curved_geometry.md)
TENSOR_CASES = [(P, g) for g in (2, 3) for P in (1, 2, 3, 4, 6)] + [(8, 4)]


@pytest.mark.parametrize("P,g", TENSOR_CASES)
def test_exported_tensor(pm, P, g):
    from pmg_dolfinx_amd import _lib

    tol = TOL_G
    p0, p1 = mesh_pair(pm, _n(P), g)
    kappa = kappa_of(p0.ncells)
    A = reference(p0, P, kappa)
    lv, layout, op = build_op(pm, p1, P, kappa)
    assert not op.is_affine()
    G = op.geometry().cpu().numpy()
    _check(f"G (P = {P}, g = {g})", _relerr(G, framed(pm, p1, P, A.G)), tol)
    assert (G[:, :, [0, 3, 5]] > 0).all()
    # the per-point path: the library's own table handed back as caller tables, in basix node order
    perm3 = pm.cell_permutation(pm.basix_node_permutation(P))
    w3 = cg.tables(P, g)[1][perm3]
    lvb = p1.level(P)
    lcells, bcells = split_cells(p1.ncells)
    dense = pm.MatFreeLaplacian(P, kappa, pm.dofmap_in_node_order(lvb.dofmap, pm.basix_node_permutation(P)), p1.xgeom,
                                p1.geom_dofmap, lcells, bcells, lvb.bc_marker, layout, node_order="basix",
                                dphi_geometry=pm.coordinate_element_table(P, g, "basix"), G_weights=w3,
                                geometry_degree=g)
    Gd = dense.geometry().cpu().numpy()  # rows in the operator's (basix) order
    _check(f"G, per-point path against the cooperative one (P = {P}, g = {g})", _relerr(Gd, G[:, perm3]), tol)
    # a nodal field and a per-cell tensor
    kq = kq_fun(p0.dof_coordinates(P))
    T = random_spd(p0.ncells, 5)
    for o in (op, dense):
        o.set_coefficient_field(_vec(pm, layout, kq))
        o.set_coefficient_tensor(T)
    want = framed(pm, p1, P, cg.with_tensor(A, T, kq).G)
    G2 = op.geometry().cpu().numpy()
    _check(f"G with field and tensor (P = {P}, g = {g})", _relerr(G2, want), tol)
    _check(f"G with field and tensor, per-point path (P = {P}, g = {g})",
           _relerr(dense.geometry().cpu().numpy(), want[:, perm3]), tol)
    # batched geometry: the same kernel on a few patches at a time, bit for bit
    for batch in (1, 3):
        _lib.call("pmg_laplacian_set_geometry_batch", op.handle, batch)
        try:
            assert np.array_equal(op.geometry().cpu().numpy(), G2)
        finally:
            _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)
    op.set_coefficient_tensor(None)
    op.set_coefficient_field(None)
    assert np.array_equal(op.geometry().cpu().numpy(), G)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exactly representable geometry
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 3, 6])
def test_trilinear_geometry_handed_over_at_higher_degree(pm, P):
    part = pm.BoxPartition(_n(P), warp=twist)
    kappa = kappa_of(part.ncells)
    lv, layout, op1 = build_op(pm, part, P, kappa)
    G1 = op1.geometry().cpu().numpy()
    lcells, bcells = split_cells(part.ncells)
    for g in (2, 3):
        x, gd = cg.trilinear_nodes(part.xgeom, part.geom_dofmap, g)  # one node set per cell
        op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, x, gd, lcells, bcells, lv.bc_marker, layout, geometry_degree=g)
        _check(f"G of trilinear cells as g = {g}", _relerr(op.geometry().cpu().numpy(), G1), TOL_G)


@pytest.mark.parametrize("P", [2, 4])
def test_triquadratic_as_degree_three_equals_degree_two(pm, P):
    G = {}
    for g in (2, 3):
        part = pm.BoxPartition(_n(P), warp=cg.triquadratic, geom_degree=g)
        G[g] = build_op(pm, part, P, kappa_of(part.ncells))[2].geometry().cpu().numpy()
    _check("G of the triquadratic box, g = 3 against g = 2", _relerr(G[3], G[2]), TOL_G)


# ---------------------------------------------------------------------------------------------------------------------
# 4. affine detection
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 4])
def test_affine_detection_looks_at_every_node(pm, P):
    g = 2
    part = pm.BoxPartition(_n(P), geom_degree=g)
    kappa = kappa_of(part.ncells)
    lv, layout, op = build_op(pm, part, P, kappa)
    assert op.is_affine()
    A = reference(part, P, kappa)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    ref = A.apply(u)
    check_apply64(pm, op, layout, u, ref, "apply fp64, box as g = 2, stored", reps=1)
    op.set_geometry_mode("affine")
    check_apply64(pm, op, layout, u, ref, "apply fp64, box as g = 2, affine mode")
    # one mid-edge node of the last cell moved by 1e-3 h: parallelepiped corners, not an affine cell
    moved = part.xgeom.copy()
    node = part.geom_dofmap[-1][1]  # (0, 0, 1) of 3 x 3 x 3: the middle of the edge along z
    assert node not in part.geom_dofmap[:, cg.corners(g)]
    moved[node, 0] += 1e-3 / _n(P)[0]
    lcells, bcells = split_cells(part.ncells)
    bent = pm.MatFreeLaplacian(P, kappa, lv.dofmap, moved, part.geom_dofmap, lcells, bcells, lv.bc_marker, layout,
                               geometry_degree=g)
    assert not bent.is_affine()
    with pytest.raises(pm._lib.PmgError):
        bent.set_geometry_mode("affine")
    Ab = cg.laplacian(P, g, kappa, lv.dofmap, moved, part.geom_dofmap, lv.bc_marker)
    assert _relerr(Ab.apply(u), ref) > 1e-6
    check_apply64(pm, bent, layout, u, Ab.apply(u), "apply fp64, one mid-edge node moved", reps=1)


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 7. operator quantities on the annulus
# ---------------------------------------------------------------------------------------------------------------------

def curved_faces(part, P):
    """The exterior facets on r = 1 and r = 2 (the box's faces x = 0 and x = 1), whatever the cells' frames: a facet
    whose corner points lie on the circle and whose other points stay within the geometry's own error of it (a chord
    of a g = 1 cell of the coarsest mesh is 0.07 inside r = 2; the other faces reach from r = 1 to r = 2)."""
    fc, fl = part.exterior_facets()
    pts = part.facet_point_coordinates(P, fc, fl)
    r = np.hypot(pts[..., 0], pts[..., 1])

    def on_circle(R):
        return (np.abs(r - R).min(axis=1) < 1e-9) & (np.abs(r - R).max(axis=1) < 0.1)

    inner, outer = on_circle(1.0), on_circle(2.0)
    on = inner | outer
    return fc[on], fl[on], pts[on], outer[on]


@pytest.mark.parametrize("form", ["coloured", "merged"])
@pytest.mark.parametrize("P,g", [(2, 2), (2, 3), (4, 2), (4, 3)])
def test_operator_quantities(pm, P, g, form):
    p0, p1 = mesh_pair(pm, _n(P), g)
    kappa = kappa_of(p0.ncells)
    l0 = p0.level(P)
    coords = p0.dof_coordinates(P)
    marker = (l0.bc_marker.astype(bool) & (coords[:, 2] < 1e-12)).astype(np.int8)  # Dirichlet on z = 0 only
    assert 0 < marker.sum() < l0.bc_marker.sum()
    A = reference(p0, P, kappa, marker)
    lv, layout, op = build_op(pm, p1, P, kappa, marker=marker, form=form)
    tag = f"(P = {P}, g = {g}, {form})"
    u = np.random.default_rng(10 + P).standard_normal(lv.ndofs)
    check_apply64(pm, op, layout, u, A.apply(u), f"apply fp64 {tag}")
    check_apply32(op, u, A.apply(_f32(u)), marker, f"apply fp32 {tag}")
    op.compute_diag_inverse()
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    _check(f"diag_inverse {tag}", _relerr(d.data_copy(), A.diag_inverse()), TOL)
    # load vector
    assert _relerr(p1.dof_coordinates(P), coords) < 1e-13
    fv = np.sin(2 * coords[:, 0]) * np.cos(coords[:, 1]) + coords[:, 2]
    b = pm.Vector(layout)
    b.set(5.0)
    op.assemble_rhs(_vec(pm, layout, fv), b)
    want = cg.mass_vector(P, g, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, marker, f=fv)
    _check(f"assemble_rhs {tag}", _relerr(b.data_copy(), want), TOL)
    # reaction, through an apply
    sigma = np.random.default_rng(6).uniform(0.0, 4.0, p0.ncells)
    op.set_reaction(sigma)
    dr = cg.mass_vector(P, g, sigma, l0.dofmap, p0.xgeom, p0.geom_dofmap, marker)
    assert dr.max() > 0
    check_apply64(pm, op, layout, u, A.apply(u) + dr * u, f"apply fp64 with reaction {tag}", reps=1)
    op.set_reaction(None)
    # Neumann and Robin data on the curved faces r = 1 and r = 2
    c0, f0, pts0, _ = curved_faces(p0, P)
    c1, f1, pts1, _ = curved_faces(p1, P)
    assert c0.size == c1.size == 2 * _n(P)[1] * _n(P)[2] and not np.array_equal(f0, f1)
    nf = (P + 1) ** 2
    b0 = np.random.default_rng(4).standard_normal(lv.ndofs)
    bv = _vec(pm, layout, b0)
    op.assemble_neumann(c1, f1, h_fun(pts1.reshape(-1, 3)).reshape(-1, nf), bv)
    want = cg.facet_vector(P, g, l0.dofmap, p0.xgeom, p0.geom_dofmap, c0, f0, h_fun(pts0.reshape(-1, 3)), marker)
    assert np.abs(want).max() > 1e-3
    _check(f"assemble_neumann {tag}", _relerr(bv.data_copy() - b0, want), TOL)
    op.set_robin(c1, f1, alpha_fun(pts1.reshape(-1, 3)).reshape(-1, nf))
    dR = cg.facet_vector(P, g, l0.dofmap, p0.xgeom, p0.geom_dofmap, c0, f0, alpha_fun(pts0.reshape(-1, 3)), marker)
    assert dR.max() > 0
    check_apply64(pm, op, layout, u, A.apply(u) + dR * u, f"apply fp64 with Robin {tag}", reps=1)
    op.set_robin(None, None, None)
    # lifting against the dense unconstrained matrix
    m = marker.astype(bool)
    Kfree = reference(p0, P, kappa, np.zeros_like(marker)).assemble_csr()
    rng = np.random.default_rng(8)
    gv = np.where(m, rng.standard_normal(lv.ndofs), np.nan)
    rhs0 = rng.standard_normal(lv.ndofs)
    lift = Kfree @ np.where(m, gv, 0.0)
    bv = _vec(pm, layout, rhs0)
    op.apply_lifting(_vec(pm, layout, gv), bv)
    got = bv.data_copy()
    assert np.array_equal(got[m], rhs0[m]) and _relerr((rhs0 - lift)[~m], rhs0[~m]) > 1e-3
    _check(f"apply_lifting {tag}", _relerr(got[~m], (rhs0 - lift)[~m]), TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 6. integrals
# ---------------------------------------------------------------------------------------------------------------------

def test_volume_and_area_of_the_annulus(pm):
    P, n = 4, (2, 3, 2)
    err = {}
    for g in (1, 2, 3, 4):
        part = pm.BoxPartition(n, warp=cg.quarter_annulus, geom_degree=g,
                               cell_frames=np.random.default_rng(g).integers(0, 48, n))
        lv = part.level(P)
        nomark = np.zeros(lv.ndofs, dtype=np.int8)
        _, layout, op = build_op(pm, part, P, 1.0, marker=nomark)
        b = pm.Vector(layout)
        op.assemble_rhs(_vec(pm, layout, np.ones(lv.ndofs)), b)
        vol = b.data_copy().sum()
        ref = cg.mass_weights(P, g, part.xgeom, part.geom_dofmap).sum()
        _check(f"volume against the reference's (g = {g})", abs(vol - ref) / (0.75 * np.pi), TOL)
        err[g] = abs(vol - 0.75 * np.pi) / (0.75 * np.pi)
        # unit flux through r = 2
        fc, fl, pts, outer = curved_faces(part, P)
        bv = pm.Vector(layout)
        bv.set(0.0)
        op.assemble_neumann(fc[outer], fl[outer], np.ones((int(outer.sum()), (P + 1) ** 2)), bv)
        area = cg.facet_weights(P, g, part.xgeom, part.geom_dofmap, fc[outer], fl[outer]).sum()
        _check(f"area of r = 2 against the reference's (g = {g})", abs(bv.data_copy().sum() - area) / area, TOL)
        print(f"curved geometry: g = {g}: volume error {err[g]:.2e}, area error {abs(area - np.pi) / np.pi:.2e}")
    for g in (1, 2, 3):
        assert err[g] > 100 * err[g + 1], err


# ---------------------------------------------------------------------------------------------------------------------
# 8. the assembled matrix, the cycle, AMG
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,g", [(1, 2), (2, 2), (3, 3)])
def test_matrix_operator(pm, P, g):
    p0, p1 = mesh_pair(pm, (3, 4, 6) if P <= 2 else (2, 3, 3), g)
    kappa = kappa_of(p0.ncells)
    A = reference(p0, P, kappa)
    lv, layout, op = build_op(pm, p1, P, kappa)
    M = pm.MatrixOperator(op)
    ref, got = A.assemble_csr(), M.to_scipy()
    diff = abs(got - ref)
    _check(f"MatrixOperator entries (P = {P}, g = {g})", (diff.max() if diff.nnz else 0.0) / np.abs(ref.data).max(),
           TOL)
    u = np.random.default_rng(100 + P).standard_normal(lv.ndofs)
    x, y = _vec(pm, layout, u), pm.Vector(layout)
    M(x, y)
    _check(f"MatrixOperator product (P = {P}, g = {g})", _relerr(y.data_copy(), A.apply(u)), TOL)


# (the degree-1 level has 9 * 9 * 13 = 1053 dofs: the smallest box of this shape on which the AMG coarsens at all)
CYCLE_N, CYCLE_ORDERS, CYCLE_K, CYCLE_G = (8, 8, 12), (1, 2, 4), 3, 2


@pytest.fixture(scope="module")
def cycle(pm):
    """The device hierarchy on the annulus at g = 2 and the oracle's cycle on the same (frame-free) mesh, its
    smoothers given the device's eigenvalue bounds so that the cycle's arithmetic alone is compared."""
    from oracle import pmg_oracle as po

    fr = np.random.default_rng(216).integers(0, 48, CYCLE_N)
    h = pm.PoissonHierarchy(CYCLE_N, CYCLE_ORDERS, kappa=2.0, cheb_its=CYCLE_K, warp=cg.quarter_annulus,
                            cell_frames=fr, geom_degree=CYCLE_G)
    assert h.geom_degree == CYCLE_G and all(op.geometry_degree() == CYCLE_G for op in h.operators)
    p0 = pm.BoxPartition(CYCLE_N, warp=cg.quarter_annulus, geom_degree=CYCLE_G)
    ops = [reference(p0, P, 2.0) for P in CYCLE_ORDERS]
    sm = [po.Chebyshev(e, CYCLE_K) for e in h.eig_ranges]
    it = [po.Interpolator(CYCLE_ORDERS[l], CYCLE_ORDERS[l + 1], ops[l].dofmap, ops[l + 1].dofmap, ops[l].ndofs,
                          ops[l + 1].ndofs) for l in range(len(ops) - 1)]
    mg = po.MultigridPreconditioner(ops, sm, it, p0.level(CYCLE_ORDERS[0]).bc_marker)
    c = p0.dof_coordinates(CYCLE_ORDERS[-1])
    fv = 29 * np.pi**2 * np.sin(2 * np.pi * c[:, 0]) * np.sin(3 * np.pi * c[:, 1]) * np.sin(4 * np.pi * c[:, 2])
    b = cg.mass_vector(CYCLE_ORDERS[-1], CYCLE_G, ops[-1].kappa, ops[-1].dofmap, p0.xgeom, p0.geom_dofmap,
                       p0.level(CYCLE_ORDERS[-1]).bc_marker, f=fv)
    # the eigenvalue bound of the oracle's own estimate, level by level
    for got, A in zip(h.eig_ranges, ops):
        ref, _ = po.estimate_eig_range(A, A.ndofs)
        _check("cycle: eigenvalue bound", abs(got[1] - ref[1]) / ref[1], 1e-8)
    return h, ops, mg, b


def test_cycle_eager_graph_and_fused_restriction(pm, cycle):
    h, ops, mg, b = cycle
    _check("cycle: right-hand side", _relerr(h.rhs[-1].data_copy(), b), TOL)
    xo, ref = np.zeros_like(b), []
    for _ in range(2):
        xo = mg.apply(b, xo, compute_rnorm=True)
        ref.append((xo.copy(), mg.rnorm))
    assert ref[1][1] < 0.5 * ref[0][1]
    for fused in (None, False):
        h.mg.set_fused_restriction(fused)
        for graph in (False, True):
            h.mg.set_graph(graph)
            x = h.new_vector()
            x.set(0.0)
            for i in range(2):
                rn = h.mg.apply(h.rhs[-1], x, verbose=True)
                _check(f"cycle: two V-cycles ({'graph' if graph else 'eager'}, fused restriction "
                       f"{'automatic' if fused is None else 'off'})", _relerr(x.data_copy(), ref[i][0]), TOL_CYCLE)
                assert abs(rn - ref[i][1]) < 1e-9 * ref[i][1]
            if fused is False:
                assert h.mg.fused_restrictions() == 0
    h.mg.set_graph(False)
    h.mg.set_fused_restriction(None)


def test_amg_on_the_degree_one_level(pm, cycle):
    from oracle.amg_oracle import AmgCycle

    h, ops, mg, b = cycle
    op, layout, lv = h.operators[0], h.layouts[0], h.levels[0]
    k = 2
    amg = pm.AmgSolver(op, smoother_iterations=k)
    L = amg.num_levels()
    assert L >= 2
    As = [amg.export(l, "A") for l in range(L)]
    Ps = [amg.export(l, "P") for l in range(L - 1)]
    ref = ops[0].assemble_csr()
    _check("AMG: level 0 against the reference's matrix", abs(As[0] - ref).max() / abs(ref).max(), TOL)
    refc = AmgCycle(As, Ps, [amg.level_info(l)["lambda_max"] for l in range(L)], k)
    bc = lv.bc_marker.astype(bool)
    rhs = np.random.default_rng(1).standard_normal(lv.ndofs)
    rhs[bc] = 0.0
    x = pm.Vector(layout)
    x.set(7.0)
    amg.cycle(x, _vec(pm, layout, rhs))
    want = refc.cycle(rhs)
    _check("AMG: cycle against the numpy restatement", np.abs(x.data_copy() - want).max() / np.abs(want).max(), TOL_AMG)


# ---------------------------------------------------------------------------------------------------------------------
# 9. the O-grid with its outer blocks on the sphere, g = 2: irregular edges, left-handed blocks, no tensor grid
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_cell", [False, True], ids=["nodes-stored-once", "nodes-per-cell"])
@pytest.mark.parametrize("P", [2, 4, 6])
def test_ogrid_on_the_sphere(pm, P, per_cell):
    import multiblock_mesh as mb

    g = 2
    mesh = mb.ogrid(6 if P <= 2 else (3 if P <= 4 else 2))  # the sizes L / M / S of tests/test_gpu_multiblock.py
    x, gd = cg.multiblock_nodes(mesh, g, warp=cg.onto_the_sphere, per_cell=per_cell)
    assert (gd.max() + 1 == x.shape[0]) and (x.shape[0] == gd.size) == per_cell
    assert abs(np.linalg.norm(x, axis=1).max() - 1.0) < 1e-14  # the outer faces' nodes lie on the sphere
    kappa = kappa_of(mesh.ncells)
    lv = mesh.level(P)
    layout = pm.make_layout(lv)
    lcells, bcells = split_cells(mesh.ncells)
    op = pm.MatFreeLaplacian(P, kappa, lv.dofmap, x, gd, lcells, bcells, lv.bc_marker, layout, geometry_degree=g)
    A = cg.laplacian(P, g, kappa, lv.dofmap, x, gd, lv.bc_marker)
    assert (np.linalg.det(cg.jacobians(P, g, x, gd)) < 0).any()  # left-handed blocks stay left-handed
    # the volume converges to the ball's: a curved boundary, not the cube's
    vol = cg.mass_weights(P, g, x, gd).sum()
    assert abs(vol - 4.0 * np.pi / 3.0) < 0.02 * 4.0 * np.pi / 3.0
    tag = f"O-grid (P = {P}, {'per cell' if per_cell else 'once'})"
    _check(f"G {tag}", _relerr(op.geometry().cpu().numpy(), A.G), TOL_G)
    u = np.random.default_rng(10 + P).standard_normal(lv.ndofs)
    check_apply64(pm, op, layout, u, A.apply(u), f"apply fp64 {tag}")
    op.compute_diag_inverse()
    d = pm.Vector(layout)
    op.get_diag_inverse(d)
    _check(f"diag_inverse {tag}", _relerr(d.data_copy(), A.diag_inverse()), TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 10. two ranks as two threads on the one GPU: the annulus cut in x
# ---------------------------------------------------------------------------------------------------------------------

def test_two_ranks(pm):
    import threading

    from oracle import pmg_oracle as po
    from test_gpu_distributed import _ThreadComm, _ThreadWorld

    n, dims, orders, g, world = (4, 3, 4), (2, 1, 1), (1, 2, 4), 2, 2
    fr = np.random.default_rng(48).integers(0, 48, n)
    p0 = pm.BoxPartition(n, warp=cg.quarter_annulus, geom_degree=g)
    ops = [reference(p0, P, 2.0) for P in orders]
    ug = np.random.default_rng(11).standard_normal(ops[-1].ndofs)
    want = ops[-1].apply(ug)
    W = _ThreadWorld(world)
    res, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                comm = _ThreadComm(W, rank)
                H = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=3, proc_dims=dims, rank=rank, size=world,
                                        comm=comm, warp=cg.quarter_annulus, cell_frames=fr, geom_degree=g)
                lv, layout, op = H.levels[-1], H.layouts[-1], H.operators[-1]
                out = {"eig": H.eig_ranges, "num_ghosts": lv.num_ghosts}
                xl = np.zeros(lv.ndofs)
                xl[: lv.size_local] = ug[lv.local_to_global[: lv.size_local]]  # ghosts stale
                x, y = _vec(pm, layout, xl), pm.Vector(layout)
                op(x, y)
                ref = want[lv.local_to_global[: lv.size_local]]
                out["apply"] = float(np.abs(y.data_copy()[: lv.size_local] - ref).max() / np.abs(want).max())
                out["rhs"] = H.rhs[-1].data_copy()[: lv.size_local]
                W.wait()
                xv = H.new_vector()
                xv.set(0.0)
                out["rnorm"] = H.mg.apply(H.rhs[-1], xv, verbose=True)
                out["iterate"] = xv.data_copy()[: lv.size_local]
                out["l2g"] = lv.local_to_global[: lv.size_local]
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
    sm = [po.Chebyshev(e, 3) for e in res[0]["eig"]]
    it = [po.Interpolator(orders[l], orders[l + 1], ops[l].dofmap, ops[l + 1].dofmap, ops[l].ndofs, ops[l + 1].ndofs)
          for l in range(len(ops) - 1)]
    mg = po.MultigridPreconditioner(ops, sm, it, p0.level(orders[0]).bc_marker)
    b = np.zeros(ops[-1].ndofs)
    for out in res:
        assert out["num_ghosts"] > 0 and out["eig"] == res[0]["eig"]
        _check("two ranks: apply", out["apply"], TOL)
        b[out["l2g"]] = out["rhs"]
    c = p0.dof_coordinates(orders[-1])
    fv = 29 * np.pi**2 * np.sin(2 * np.pi * c[:, 0]) * np.sin(3 * np.pi * c[:, 1]) * np.sin(4 * np.pi * c[:, 2])
    bref = cg.mass_vector(orders[-1], g, ops[-1].kappa, ops[-1].dofmap, p0.xgeom, p0.geom_dofmap,
                          p0.level(orders[-1]).bc_marker, f=fv)
    _check("two ranks: right-hand side", _relerr(b, bref), TOL)
    xo = mg.apply(bref, np.zeros_like(bref), compute_rnorm=True)
    for out in res:
        _check("two ranks: one V-cycle", np.abs(out["iterate"] - xo[out["l2g"]]).max() / np.abs(xo).max(), TOL_CYCLE)
        assert abs(out["rnorm"] - mg.rnorm) < 1e-8 * mg.rnorm


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals: a message and a NULL handle
# ---------------------------------------------------------------------------------------------------------------------

def test_refusals(pm):
    import ctypes as C

    from pmg_dolfinx_amd import _lib

    P, g = 2, 2
    part = pm.BoxPartition((2, 2, 3), geom_degree=g)
    lv, layout, good = build_op(pm, part, P, 1.0)
    lc, bc_ = split_cells(part.ncells)

    def create(geom_degree, gd):
        h = _lib.vp(12345)  # (overwritten with NULL by a refusal)
        rc = _lib.lib().pmg_laplacian_create_curved(
            C.byref(h), layout.handle, P, part.ncells, _lib.ptr(good.kappa), _lib.ptr(good.dofmap),
            _lib.ptr(good.xgeom), int(good.xgeom.numel() // 3), geom_degree, _lib.ptr(gd), None, None,
            lc.ctypes.data_as(_lib.c_ip), lc.size, bc_.ctypes.data_as(_lib.c_ip), bc_.size, _lib.ptr(good.bc_marker),
            0, None, _lib.current_stream())
        return rc, h.value, _lib.lib().pmg_last_error().decode()

    for bad in (0, 5):
        rc, h, msg = create(bad, good.geom_dofmap)
        assert rc != 0 and not h and "1..4" in msg and "geometry degree" in msg
    gd = good.geom_dofmap.clone()
    gd.view(-1)[-1] = part.xgeom.shape[0]  # the last node of the last cell
    rc, h, msg = create(g, gd)
    assert rc != 0 and not h and "geometry dofmap entry" in msg and "out of range" in msg
    gd.view(-1)[-1] = -1
    rc, h, msg = create(g, gd)
    assert rc != 0 and not h and "out of range" in msg
    rc, h, msg = create(g, good.geom_dofmap)
    assert rc == 0 and h
    _lib.lib().pmg_laplacian_destroy(_lib.vp(h))
