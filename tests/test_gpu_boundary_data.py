"""Boundary data on the device: pmg_laplacian_apply_lifting, pmg_laplacian_set_bc, pmg_laplacian_assemble_neumann.

The CPU truth for the lifting is ``A_free @ where(bc, g - x0, 0)`` with ``A_free`` the oracle's operator built with an
all-zero marker (with a coefficient field its tensor is scaled as tests/test_gpu_coefficient_field.py does); for the
Neumann load it is tests/boundary_data_reference.py, which takes adj(J) from numpy.linalg.  The bound is the suite's
bound for an apply against the oracle, max|a-b| / max|b| <= 1e-12; nothing is compared bit for bit that went through
an atomic sum."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12
MAPS = {"warp": ref.warp, "twist": ref.twist, "box": None}


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


def _level(pm, n, P, wf, kappa=2.0, marker=None, node_order="ascending"):
    part = pm.BoxPartition(n, warp=wf)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    bc = lv.bc_marker if marker is None else np.ascontiguousarray(marker, dtype=np.int8)
    dm = lv.dofmap
    if node_order != "ascending":
        dm = pm.dofmap_in_node_order(lv.dofmap, pm.basix_node_permutation(P))
    op = pm.MatFreeLaplacian(P, kappa, dm, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bc, layout,
                             node_order=node_order)
    return part, lv, layout, op, bc


def _free_oracle(P, kappa, lv, part, kq=None):
    """The unconstrained operator: the oracle with an all-zero marker."""
    from oracle import pmg_oracle as po

    A = po.Laplacian(P, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, np.zeros(lv.ndofs, dtype=np.int8))
    if kq is not None:
        A.G *= kq[A.dofmap][:, :, None]
        A._diag = None
    return A


def _data(lv, bc, seed, with_x0=True):
    """g and x0 random on marked dofs and NaN on unmarked ones, b0 random."""
    rng = np.random.default_rng(seed)
    m = np.asarray(bc).astype(bool)
    g = np.where(m, rng.standard_normal(lv.ndofs), np.nan)
    x0 = np.where(m, rng.standard_normal(lv.ndofs), np.nan) if with_x0 else None
    return g, x0, rng.standard_normal(lv.ndofs)


def _expected_lifting(A, bc, g, x0, b0, alpha):
    m = np.asarray(bc).astype(bool)
    lift = A.apply(np.where(m, g - (x0 if x0 is not None else 0.0), 0.0))
    return np.where(m, b0, b0 - alpha * lift)


def _check_lifting(pm, op, layout, A, bc, g, x0, b0, alpha, what=""):
    gv, bv = _vec(pm, layout, g), _vec(pm, layout, b0)
    xv = _vec(pm, layout, x0) if x0 is not None else None
    op.apply_lifting(gv, bv, x0=xv, alpha=alpha)
    torch.cuda.synchronize()
    got, want = bv.data_copy(), _expected_lifting(A, bc, g, x0, b0, alpha)
    m = np.asarray(bc).astype(bool)
    assert not np.isnan(got).any(), "a NaN of an unmarked entry reached b"
    assert np.array_equal(got[m], b0[m]), "marked rows of b were touched"
    err = _relerr(got[~m], want[~m])
    print(f"lifting {what}: max|b - expected| / max|expected| = {err:.3e}")
    assert err <= TOL
    assert _relerr(want[~m], b0[~m]) > 1e-3  # the lifting is really in the expected vector
    return got


# ---- 1. lifting, every degree ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("wf", ["warp", "twist"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_lifting_all_degrees(pm, P, wf):
    """(3, 2, 2) cells: cells with one, two and three boundary faces; at P <= 2 several cells share a workgroup and
    the last one is partly filled (12 cells: 8 + 4 at P = 1, 3 per workgroup at P = 2)."""
    n = (3, 2, 2)
    kappa = np.random.default_rng(40 + P).uniform(0.5, 2.0, 12)
    part, lv, layout, op, bc = _level(pm, n, P, MAPS[wf], kappa=kappa)
    g, x0, b0 = _data(lv, bc, 10 * P + len(wf))
    A = _free_oracle(P, kappa, lv, part)
    assert op.lift_cell_count() == -1
    _check_lifting(pm, op, layout, A, bc, g, x0, b0, -0.7, f"P = {P}, {wf}")
    assert op.lift_cell_count() == 12  # every cell of this mesh touches the boundary


# ---- 2. a marker that is not the boundary ---------------------------------------------------------------------------


def test_marker_that_is_not_the_boundary(pm):
    P, n = 3, (3, 3, 3)
    part = pm.BoxPartition(n, warp=ref.twist)
    lv = part.level(P)
    flat = pm.BoxPartition(n).dof_coordinates(P)  # reference positions: which dofs lie on x = 0
    marker = (np.abs(flat[:, 0]) < 1e-12).astype(np.int8)
    centre = 13  # cell (1, 1, 1)
    lone = lv.dofmap[centre][(1 * 4 + 2) * 4 + 1]  # a cell-interior node of the interior cell
    assert (lv.dofmap == lone).sum() == 1 and not lv.bc_marker[lone]
    marker[lone] = 1
    part, lv, layout, op, bc = _level(pm, n, P, ref.twist, marker=marker)
    g, x0, b0 = _data(lv, bc, 5)
    A = _free_oracle(P, 2.0, lv, part)
    got = _check_lifting(pm, op, layout, A, bc, g, x0, b0, 1.0, "face x = 0 and a lone interior dof")
    touching = np.nonzero(marker.astype(bool)[lv.dofmap].any(axis=1))[0]
    assert sorted(touching.tolist()) == sorted([c for c in range(27) if part.cell_coords[c][0] == 0] + [centre])
    assert op.lift_cell_count() == touching.size == 10
    # seen through the result: rows next to the lone dof change, rows of untouched cells stay bit-equal
    m = marker.astype(bool)
    near = np.setdiff1d(lv.dofmap[centre], np.nonzero(m)[0])
    changed = got[near] != b0[near]  # (a node that shares no grid line with the lone dof has an exact zero entry)
    assert changed.sum() >= 9 and near.size == 63
    in_list = np.zeros(lv.ndofs, dtype=bool)
    in_list[lv.dofmap[touching].ravel()] = True
    assert (~in_list).sum() > 0 and np.array_equal(got[~in_list], b0[~in_list])


# ---- 3. modes -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", [2, 4])
def test_lifting_follows_the_coefficient_field(pm, P):
    n = (3, 2, 2)
    part, lv, layout, op, bc = _level(pm, n, P, ref.twist)
    kq = np.random.default_rng(60 + P).uniform(0.5, 2.0, lv.ndofs)
    g, x0, b0 = _data(lv, bc, 61)
    plain = _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part), bc, g, x0, b0, 1.0, "before the field")
    op.set_coefficient_field(_vec(pm, layout, kq))
    field = _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part, kq), bc, g, x0, b0, 1.0, "with the field")
    assert _relerr(field, plain) > 1e-2
    op.set_coefficient_field(None)
    again = _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part), bc, g, x0, b0, 1.0, "field cleared")
    assert _relerr(again, plain) <= 1e-14


@pytest.mark.parametrize("P", [2, 4])
def test_lifting_with_batched_geometry(pm, P):
    from pmg_dolfinx_amd import _lib

    n = (4, 4, 4)
    part, lv, layout, op, bc = _level(pm, n, P, ref.warp)
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 8)  # far fewer cells than the mesh: no resident tensor
    kq = np.random.default_rng(70 + P).uniform(0.5, 2.0, lv.ndofs)
    op.set_coefficient_field(_vec(pm, layout, kq))
    g, x0, b0 = _data(lv, bc, 71)
    _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part, kq), bc, g, x0, b0, 0.5, "batched geometry")
    assert op.lift_cell_count() == 64 - 8


@pytest.mark.parametrize("P", [2, 4])
def test_lifting_in_affine_mode_and_without_x0(pm, P):
    n = (3, 2, 2)
    part, lv, layout, op, bc = _level(pm, n, P, None)
    assert op.is_affine()
    op.set_geometry_mode("affine")
    g, _, b0 = _data(lv, bc, 81, with_x0=False)
    _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part), bc, g, None, b0, 1.0, "affine mode, x0 = None")


@pytest.mark.parametrize("P", [2, 4])
def test_lifting_in_basix_node_order(pm, P):
    n = (3, 2, 2)
    part, lv, layout, op, bc = _level(pm, n, P, ref.twist, node_order="basix")
    g, x0, b0 = _data(lv, bc, 91)
    # vectors and the marker are indexed by dof number: the oracle never sees the basix order
    _check_lifting(pm, op, layout, _free_oracle(P, 2.0, lv, part), bc, g, x0, b0, 1.0, "basix node order")


@pytest.mark.parametrize("P", [2, 4])
def test_lifting_agrees_with_a_second_unconstrained_operator(pm, P):
    """The old route: a second complete operator with an all-zero marker applied to the masked g."""
    n = (3, 2, 2)
    part, lv, layout, op, bc = _level(pm, n, P, ref.warp)
    _, _, _, op_free, _ = _level(pm, n, P, ref.warp, marker=np.zeros(lv.ndofs, dtype=np.int8))
    g, _, _ = _data(lv, bc, 95, with_x0=False)
    m = bc.astype(bool)
    gm = _vec(pm, layout, np.where(m, g, 0.0))
    Ag = pm.Vector(layout)
    op_free(gm, Ag)
    b = pm.Vector(layout)
    b.set(0.0)
    op.apply_lifting(_vec(pm, layout, g), b, alpha=-1.0)  # b = + A g on the unmarked rows
    got, old = b.data_copy(), Ag.data_copy()
    assert _relerr(got[~m], old[~m]) <= TOL and np.all(got[m] == 0.0)


# ---- 4. set_bc ------------------------------------------------------------------------------------------------------


def _check_set_bc(pm, op, layout, bc, n, seed):
    rng = np.random.default_rng(seed)
    m = np.asarray(bc).astype(bool)
    g = np.where(m, rng.standard_normal(n), np.nan)
    x0 = np.where(m, rng.standard_normal(n), np.nan)
    b0 = rng.standard_normal(n)
    for alpha, xx in ((1.0, None), (-0.7, x0)):
        gv, bv = _vec(pm, layout, g), _vec(pm, layout, b0)
        xv = _vec(pm, layout, xx) if xx is not None else None
        op.set_bc(gv, bv, x0=xv, alpha=alpha)
        want = torch.from_numpy(b0).cuda()
        mt = torch.from_numpy(m).cuda()
        val = alpha * (gv.data - xv.data) if xv is not None else alpha * gv.data
        want[mt] = val[mt]
        assert torch.equal(bv.data, want)
        assert not torch.isnan(bv.data).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_set_bc_lengths(pm, n):
    """An operator without cells over a layout of n dofs: set_bc is element-wise over the marker."""
    layout = pm.Layout(n)
    bc = (np.random.default_rng(n).uniform(size=n) < 0.5).astype(np.int8)
    bc[n - 1] = 1  # the last entry is written
    bc[0] = 1 if n == 1 else 0
    empty_i = np.zeros(0, dtype=np.int32)
    op = pm.MatFreeLaplacian(1, 2.0, empty_i, np.zeros(0), empty_i, empty_i, empty_i, bc, layout)
    _check_set_bc(pm, op, layout, bc, n, 100 + n)


def test_set_bc_on_a_level(pm):
    part, lv, layout, op, bc = _level(pm, (3, 2, 2), 3, ref.twist)
    _check_set_bc(pm, op, layout, bc, lv.ndofs, 7)


# ---- 5. Neumann load ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_neumann_all_degrees(pm, P):
    n = (2, 2, 2)
    flat = pm.BoxPartition(n).dof_coordinates(P)
    marker = (np.abs(flat[:, 0]) < 1e-12).astype(np.int8)  # the face x = 0
    part, lv, layout, op, bc = _level(pm, n, P, ref.warp, marker=marker)
    cells, facets = part.exterior_facets()
    rng = np.random.default_rng(200 + P)
    order = rng.permutation(cells.size)
    cells, facets = cells[order], facets[order]
    h = rng.standard_normal((cells.size, (P + 1) ** 2))
    b0 = rng.standard_normal(lv.ndofs)
    b = _vec(pm, layout, b0)
    op.assemble_neumann(cells, facets, h, b)
    want = b0 + ref.neumann_reference(part, P, lv.dofmap, cells, facets, h, marker, lv.ndofs)
    got = b.data_copy()
    m = marker.astype(bool)
    assert np.array_equal(got[m], b0[m])  # marked rows untouched
    err = _relerr(got, want)
    print(f"Neumann load P = {P}: {err:.3e}")
    assert err <= TOL
    assert _relerr(want, b0) > 1e-3


@pytest.mark.parametrize("P", [1, 4, 8])
def test_neumann_unit_flux_gives_the_area_of_the_box(pm, P):
    part, lv, layout, op, bc = _level(pm, (2, 2, 2), P, None, marker=np.zeros((2 * P + 1) ** 3, dtype=np.int8))
    cells, facets = part.exterior_facets()
    b = pm.Vector(layout)
    b.set(0.0)
    op.assemble_neumann(cells, facets, np.ones((cells.size, (P + 1) ** 2)), b)
    assert abs(b.data_copy().sum() - 6.0) <= 1e-13
    op.assemble_neumann(cells[:0], facets[:0], np.zeros((0, (P + 1) ** 2)), b)  # nfacets == 0: a no-op
    assert abs(b.data_copy().sum() - 6.0) <= 1e-13


def test_neumann_facet_numbering_face_by_face(pm):
    """The six local facets of a single (twisted) cell, one call each and all in one list."""
    P = 3
    marker = np.zeros(64, dtype=np.int8)
    part, lv, layout, op, bc = _level(pm, (1, 1, 1), P, ref.twist, marker=marker)
    rng = np.random.default_rng(3)
    h = rng.standard_normal((6, 16))
    cells, facets = np.zeros(6, dtype=np.int32), np.arange(6, dtype=np.int8)
    for f in range(6):
        b = pm.Vector(layout)
        b.set(0.0)
        op.assemble_neumann(cells[f: f + 1], facets[f: f + 1], h[f: f + 1], b)
        want = ref.neumann_reference(part, P, lv.dofmap, cells[f: f + 1], facets[f: f + 1], h[f: f + 1], marker, 64)
        got = b.data_copy()
        on_face = np.zeros(64, dtype=bool)
        on_face[lv.dofmap[0][pm.facet_nodes(P, f)]] = True
        assert np.all(got[~on_face] == 0.0) and np.all(got[on_face] != 0.0)
        assert _relerr(got, want) <= TOL, f
    b = pm.Vector(layout)
    b.set(0.0)
    op.assemble_neumann(cells, facets, h, b)
    assert _relerr(b.data_copy(), ref.neumann_reference(part, P, lv.dofmap, cells, facets, h, marker, 64)) <= TOL


# ---- 6. refusals ----------------------------------------------------------------------------------------------------


def test_refusals_write_nothing(pm):
    from pmg_dolfinx_amd import _lib
    from pmg_dolfinx_amd._lib import current_stream, ptr

    P = 2
    part = pm.BoxPartition((3, 2, 2), warp=ref.twist)
    lv = part.level(P)
    layout = pm.make_layout(lv)
    # cell 11 is in neither cell list: the operator does not know it
    listed = np.arange(11, dtype=np.int32)
    op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, listed, np.zeros(0, dtype=np.int32),
                             lv.bc_marker, layout)
    g, x0, b0 = _data(lv, lv.bc_marker, 1)
    gv, xv, bv = _vec(pm, layout, g), _vec(pm, layout, x0), _vec(pm, layout, b0)
    before = bv.data.clone()
    nf = (P + 1) ** 2
    h = torch.ones(4 * nf, dtype=torch.float64, device="cuda")
    cells, facets = np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 2, 4, 0], dtype=np.int8)
    ip, bp = _lib.c_ip, _lib.c_bp
    s = current_stream()

    def refused(name, *args):
        rc = getattr(_lib.lib(), name)(*args)
        assert rc == -1, (name, rc)  # PMG_ERR_INVALID
        assert name.encode() in _lib.lib().pmg_last_error()
        torch.cuda.synchronize()
        assert torch.equal(bv.data, before), name

    H = op.handle
    refused("pmg_laplacian_apply_lifting", None, ptr(gv.data), None, 1.0, ptr(bv.data), s)
    refused("pmg_laplacian_apply_lifting", H, None, None, 1.0, ptr(bv.data), s)
    refused("pmg_laplacian_apply_lifting", H, ptr(gv.data), None, 1.0, None, s)
    refused("pmg_laplacian_apply_lifting", H, ptr(bv.data), None, 1.0, ptr(bv.data), s)                # b aliases g
    refused("pmg_laplacian_apply_lifting", H, ptr(gv.data), ptr(bv.data), 1.0, ptr(bv.data), s)        # b aliases x0
    refused("pmg_laplacian_set_bc", None, ptr(gv.data), None, 1.0, ptr(bv.data), s)
    refused("pmg_laplacian_set_bc", H, None, None, 1.0, ptr(bv.data), s)
    refused("pmg_laplacian_set_bc", H, ptr(gv.data), None, 1.0, None, s)
    refused("pmg_laplacian_set_bc", H, ptr(bv.data), None, 1.0, ptr(bv.data), s)
    refused("pmg_laplacian_set_bc", H, ptr(gv.data), ptr(bv.data), 1.0, ptr(bv.data), s)

    def neumann(c, f, hh=h, handle=H, b=bv.data, count=None):
        return ("pmg_laplacian_assemble_neumann", handle, len(c) if count is None else count,
                c.ctypes.data_as(ip) if c is not None else None, f.ctypes.data_as(bp) if f is not None else None,
                ptr(hh) if hh is not None else None, ptr(b) if b is not None else None, s)

    refused(*neumann(cells, facets, handle=None))
    refused(*neumann(cells, facets, hh=None))
    refused(*neumann(cells, facets, b=None))
    refused(*neumann(None, facets, count=4))
    refused(*neumann(cells, None, count=4))
    for bad in (-1, part.ncells, 11):  # outside [0, ncells) twice, then a cell the operator does not list
        c = cells.copy()
        c[2] = bad
        refused(*neumann(c, facets))
    for bad in (-1, 6):
        f = facets.copy()
        f[3] = bad
        refused(*neumann(cells, f))
    # inside a stream capture: the first lifting call of an operator (it builds a list on the host), and the Neumann
    # load (it uploads lists); a capture that only held refused calls is ended and thrown away
    assert op.lift_cell_count() == -1
    side, scratch = torch.cuda.Stream(), torch.zeros(8, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)  # the capture holds one kernel of its own
            cs = current_stream()
            rc1 = _lib.lib().pmg_laplacian_apply_lifting(H, ptr(gv.data), ptr(xv.data), 1.0, ptr(bv.data), cs)
            msg1 = _lib.lib().pmg_last_error()
            rc2 = _lib.lib().pmg_laplacian_assemble_neumann(H, 4, cells.ctypes.data_as(ip), facets.ctypes.data_as(bp),
                                                            ptr(h), ptr(bv.data), cs)
            msg2 = _lib.lib().pmg_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc1 == -1 and b"stream capture" in msg1 and rc2 == -1 and b"stream capture" in msg2
    assert op.lift_cell_count() == -1
    torch.cuda.synchronize()
    assert torch.equal(bv.data, before)
    # ... and the calls work afterwards
    op.apply_lifting(gv, bv, x0=xv)
    op.assemble_neumann(cells, facets, h, bv)
    torch.cuda.synchronize()
    assert op.lift_cell_count() == 11 and not torch.equal(bv.data, before)


# ---- 7. end to end: the exactness the method promises ----------------------------------------------------------------


def _mixed_rhs(pm, part, P, op, layout, marker):
    """b from assemble_rhs + assemble_neumann + apply_lifting + set_bc, and x with set_bc(g)."""
    cells, facets = part.exterior_facets()
    u, f_over_kappa, h, marker_ref = ref.mixed_problem_data(part, P, cells, facets)
    assert np.array_equal(marker_ref, marker)
    g = _vec(pm, layout, np.where(marker.astype(bool), u, np.nan))
    b, x = pm.Vector(layout), pm.Vector(layout)
    op.assemble_rhs(_vec(pm, layout, f_over_kappa), b)
    op.assemble_neumann(cells, facets, h, b)
    op.apply_lifting(g, b)
    op.set_bc(g, b)
    x.set(0.0)
    op.set_bc(g, x)
    return u, b, x


def _oracle_cg_error(part, P, marker, u, b, max_it):
    from oracle import pmg_oracle as po

    lv = part.level(P)
    A = po.Laplacian(P, ref.KAPPA, lv.dofmap, part.xgeom, part.geom_dofmap, marker)
    cg = po.CGSolver()
    cg.set_max_iterations(max_it)
    cg.set_tolerance(1e-12)
    x = np.where(marker.astype(bool), u, 0.0)
    cg.solve(A, x, b)
    return _relerr(x, u)


@pytest.mark.parametrize("P", [2, 3, 4])
def test_mixed_problem_end_to_end(pm, P):
    """Unit box of (2, 3, 2) cells, kappa = 2, Dirichlet on x = 0, x = 1, y = 0, Neumann elsewhere, polynomial u of
    degree <= P - 1 per variable: Jacobi-CG at rtol 1e-12 returns u at the nodes.  Bound: ten times the error of the
    oracle's CGSolver on the same system with the same settings, never below 1e-11.
    Measured on an MI355X, library / oracle's CGSolver: P = 2 2.428e-13 / 2.430e-13 (40 iterations), P = 3
    4.679e-13 / 4.678e-13 (69), P = 4 4.458e-13 / 4.469e-13 (99); ten times the oracle's error is below the floor, so
    the bound in force is 1e-11."""
    n = (2, 3, 2)
    part = pm.BoxPartition(n)
    lv = part.level(P)
    marker = (lv.bc_marker.astype(bool) & ref.dirichlet_part(part.dof_coordinates(P))).astype(np.int8)
    part, lv, layout, op, bc = _level(pm, n, P, None, kappa=ref.KAPPA, marker=marker)
    op.compute_diag_inverse()
    u, b, x = _mixed_rhs(pm, part, P, op, layout, marker)
    cg = pm.CGSolver(layout)
    cg.set_max_iterations(2000)
    cg.set_tolerance(1e-12)
    its = cg.solve(op, x, b)
    err = _relerr(x.data_copy(), u)
    oerr = _oracle_cg_error(part, P, marker, u, b.data_copy(), 2000)
    bound = max(10.0 * oerr, 1e-11)
    print(f"mixed problem P = {P}: {its} iterations, max|x - u| / max|u| = {err:.3e}, oracle CG {oerr:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound


def test_mixed_problem_with_the_p_multigrid_preconditioner(pm):
    """The same problem at P = 4 with the 4 -> 2 -> 1 V-cycle as preconditioner, the partial marker on every level:
    a non-zero g must not disturb the cycle, which sees homogeneous data.  Bound as above (oracle: Jacobi-CG).
    Measured on an MI355X: 12 iterations, 4.506e-13 against the oracle's 3.918e-13; bound in force 1e-11."""
    n, P = (2, 3, 2), 4
    H = pm.PoissonHierarchy(n, (1, 2, 4), kappa=ref.KAPPA, cheb_its=3, dirichlet=ref.dirichlet_part)
    part, lv, layout, op = H.part, H.levels[-1], H.layouts[-1], H.operators[-1]
    marker = lv.bc_marker
    for lvl, Pl in zip(H.levels, (1, 2, 4)):  # partial on every level
        assert 0 < lvl.bc_marker.sum() < pm.BoxPartition(n).level(Pl).bc_marker.sum()
    u, b, x = _mixed_rhs(pm, part, P, op, layout, marker)
    cg = pm.CGSolver(layout)
    cg.set_max_iterations(200)
    cg.set_tolerance(1e-12)
    its = cg.solve(op, x, b, preconditioner=H.mg)
    err = _relerr(x.data_copy(), u)
    oerr = _oracle_cg_error(part, P, marker, u, b.data_copy(), 2000)
    bound = max(10.0 * oerr, 1e-11)
    print(f"mixed problem, p-multigrid PCG: {its} iterations, max|x - u| / max|u| = {err:.3e}, oracle CG {oerr:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound and its < 60


# ---- 8. two ranks on one GPU ----------------------------------------------------------------------------------------


def _flux(points, facet):
    return np.sin(1.0 + 2 * points[..., 0] + 3 * points[..., 1] * points[..., 2]) + 0.25 * facet


def _rank_body(rank, world, port, n, dims, P):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm
        from oracle import pmg_oracle as po

        torch.cuda.set_device(0)
        H = pm.PoissonHierarchy(n, (P,), kappa=2.0, proc_dims=dims, rank=rank, size=world, warp=ref.warp)
        part, lv, layout, op = H.part, H.levels[0], H.layouts[0], H.operators[0]
        # the single-domain truth, by global dof number
        gp = pm.BoxPartition(n, warp=ref.warp)
        glv = gp.level(P)
        A = po.Laplacian(P, 2.0, glv.dofmap, gp.xgeom, gp.geom_dofmap, np.zeros(glv.ndofs, dtype=np.int8))
        gm = glv.bc_marker.astype(bool)
        rng = np.random.default_rng(17)
        gg, gx0, gb0 = rng.standard_normal(glv.ndofs), rng.standard_normal(glv.ndofs), rng.standard_normal(glv.ndofs)
        alpha = -0.7
        want = np.where(gm, gb0, gb0 - alpha * A.apply(np.where(gm, gg - gx0, 0.0)))
        l2g, own = lv.local_to_global, lv.local_to_global[: lv.size_local]
        m = lv.bc_marker.astype(bool)
        assert np.array_equal(m, gm[l2g])
        g = np.where(m, gg[l2g], np.nan)
        g[lv.size_local:] = 777.0  # stale ghosts: the call refreshes them
        g_d, x0_d, b_d = pm.Vector(layout), pm.Vector(layout), pm.Vector(layout)
        g_d.data.copy_(torch.from_numpy(g))
        x0_d.data.copy_(torch.from_numpy(np.where(m, gx0[l2g], np.nan)))  # its ghosts are the caller's: current here
        b_d.data.copy_(torch.from_numpy(gb0[l2g]))
        op.apply_lifting(g_d, b_d, x0=x0_d, alpha=alpha)
        torch.cuda.synchronize()
        got = b_d.data_copy()[: lv.size_local]
        lift_err = float(np.abs(got - want[own]).max() / np.abs(want).max())
        ghosts_ok = bool(np.array_equal(g_d.data_copy()[lv.size_local:][m[lv.size_local:]],
                                        gg[l2g][lv.size_local:][m[lv.size_local:]]))
        # Neumann: every rank lists the exterior facets of all cells it holds
        gcells, gfacets = gp.exterior_facets()
        gcoords = gp.dof_coordinates(P)
        gh = np.stack([_flux(gcoords[glv.dofmap[c][pm.facet_nodes(P, int(f))]], int(f))
                       for c, f in zip(gcells, gfacets)])
        nwant = ref.neumann_reference(gp, P, glv.dofmap, gcells, gfacets, gh, glv.bc_marker * 0, glv.ndofs)
        cells, facets = part.exterior_facets()
        coords = part.dof_coordinates(P)
        h = np.stack([_flux(coords[lv.dofmap[c][pm.facet_nodes(P, int(f))]], int(f)) for c, f in zip(cells, facets)])
        free = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                   np.zeros(lv.ndofs, dtype=np.int8), layout)
        nb = pm.Vector(layout)
        nb.set(0.0)
        free.assemble_neumann(cells, facets, h, nb)
        torch.cuda.synchronize()
        neu_err = float(np.abs(nb.data_copy()[: lv.size_local] - nwant[own]).max() / np.abs(nwant).max())
        dist.barrier()
        return {"ghosts": int(lv.num_ghosts), "lifting": lift_err, "neumann": neu_err, "ghosts_refreshed": ghosts_ok,
                "ghost_cells_listed": bool((cells >= part.ncells_owned).any())}
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

    res = _run_ranks(_rank_worker, 2, ((3, 4, 8), (1, 1, 2), 2))
    for out in res:
        print(out)
        assert out["ghosts"] > 0 and out["ghosts_refreshed"] and out["ghost_cells_listed"]
        assert out["lifting"] <= TOL and out["neumann"] <= TOL, out


# ---- 9. drivers -----------------------------------------------------------------------------------------------------


def _run(name, *args):
    path = os.path.join(ROOT, "pmg-dolfinx_amd", "bin", name)
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cg_driver_with_lift(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    old, new = _run("cg_main", "--n", 6), _run("cg_main", "--n", 6, "--lift")
    its = [int(re.search(r"Number of iterations (\d+)", o).group(1)) for o in (old, new)]
    res = [float(re.findall(r"Chebyshev iteration \d+: residual norm = (\S+)", o)[-1]) for o in (old, new)]
    bn = [float(re.search(r"Norm of b = (\S+)", o).group(1)) for o in (old, new)]
    print(f"cg_main: iterations {its}, final residual {res}, |b| {bn}")
    assert its[0] == its[1]
    assert abs(res[0] - res[1]) <= 1e-10 * res[0]
    assert abs(bn[0] - bn[1]) <= 1e-12 * bn[0]


def test_mat_free_driver_with_lift(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run("mat_free_main", "--n", 4, "--degree", 3, "--nreps", 2, "--lift")
    assert "Lifted right-hand side: 56 of 64 cells hold a Dirichlet dof" in out
    for what in ("u", "y"):
        v = float(re.search(rf"Norm of {what} = (\S+)", out).group(1))
        assert np.isfinite(v) and v > 0
