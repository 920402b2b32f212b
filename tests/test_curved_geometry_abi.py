"""Curved cells without a GPU: the three entry points are declared, exported and bound, the Python layer refuses
arrays that do not match the geometry degree before the library is called, and ``BoxPartition(geom_degree=g)`` hands
over what the header describes -- degree 1 unchanged to the bit, shared nodes stored once, the same coordinates for a
cell on either of two ranks, dof coordinates on the discrete geometry."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import curved_geometry_reference as cg  # noqa: E402
from boundary_data_reference import twist  # noqa: E402

NAMES = ("pmg_laplacian_create_curved", "pmg_laplacian_geometry_degree", "pmg_coordinate_element_table")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared
    assert re.search(r"#define\s+PMG_MAX_GEOM_DEGREE\s+4\b", code)
    assert re.search(r"int\s+pmg_laplacian_create_curved\(pmg_laplacian\* out, pmg_layout layout, int degree, "
                     r"int32_t ncells,\s*const double\* kappa,\s*const int32_t\* dofmap, const double\* xgeom, "
                     r"int32_t npoints,\s*int geom_degree,\s*const int32_t\* geom_dofmap, const double\* dphi_geometry, "
                     r"const double\* G_weights,\s*const int32_t\* lcells, int32_t n_lcells, const int32_t\* bcells, "
                     r"int32_t n_bcells,\s*const int8_t\* bc_marker, int node_order, const int32_t\* custom_perm1d,"
                     r"\s*pmg_stream stream\);", code)
    assert re.search(r"int\s+pmg_laplacian_geometry_degree\(pmg_laplacian op\);", code)
    assert re.search(r"int\s+pmg_coordinate_element_table\(int degree, int geom_degree, int node_order,\s*"
                     r"const int32_t\* custom_perm1d,\s*double\* dphi\);", code)
    # the conventions stand next to them
    for phrase in ("ascending tensor order", "both given or both NULL", "|det J|"):
        assert phrase in src


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_geometry_degree(None) == -1
    out = np.zeros(3 * 8 * 27)
    for bad in (0, 5):
        assert lib.pmg_coordinate_element_table(1, bad, 0, None, out.ctypes.data_as(pm._lib.c_dp)) != 0
        assert b"1..4" in lib.pmg_last_error()
    assert lib.pmg_coordinate_element_table(1, 2, 0, None, None) != 0


def test_python_and_cpp_layers_carry_them(built):
    import pmg_dolfinx_amd as pm

    p = inspect.signature(pm.MatFreeLaplacian.__init__).parameters
    assert p["geometry_degree"].default == 1
    assert list(inspect.signature(pm.MatFreeLaplacian.geometry_degree).parameters) == ["self"]
    assert inspect.signature(pm.BoxPartition.__init__).parameters["geom_degree"].default == 1
    assert inspect.signature(pm.PoissonHierarchy.__init__).parameters["geom_degree"].default == 1
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "pmg_laplacian_create_curved(" in hpp and "int geometry_degree() const" in hpp
    assert "struct CurvedGeometry" in open(os.path.join(ROOT, "examples", "common", "box_mesh.hpp")).read()
    for driver in ("pmg", "mat_free"):
        assert '"--curved"' in open(os.path.join(ROOT, "examples", driver, driver + "_main.cpp")).read()


def test_python_refuses_arrays_that_do_not_match_the_degree(built):
    """Before the library is called: a stand-in layout on the CPU is enough to get there."""
    import pmg_dolfinx_amd as pm

    P, ncells = 2, 4
    layout = types.SimpleNamespace(device="cpu", total=10, handle=None)
    dofmap = np.zeros((ncells, 27), dtype=np.int32)
    x = np.zeros((200, 3))
    cells = np.arange(ncells, dtype=np.int32)

    def make(gd_width, g, dphi=None, w=None):
        return pm.MatFreeLaplacian(P, 1.0, dofmap, x, np.zeros((ncells, gd_width), dtype=np.int32), cells, cells[:0],
                                   np.zeros(10, dtype=np.int8), layout, geometry_degree=g, dphi_geometry=dphi,
                                   G_weights=w)

    for width, g in ((8, 2), (27, 1), (27, 3), (64, 2), (26, 2)):
        with pytest.raises(ValueError, match="geometry_dofmap"):
            make(width, g)
    for g in (0, 5):
        with pytest.raises(ValueError, match="geometry_degree"):
            make(8, g)
    with pytest.raises(ValueError, match="dphi_geometry"):
        make(27, 2, dphi=np.zeros((3, 27, 8)), w=np.zeros(27))
    with pytest.raises(ValueError, match="come together"):
        make(27, 2, dphi=np.zeros((3, 27, 27)))
    for bad in ((0, 2), (9, 2), (2, 0), (2, 5)):
        with pytest.raises(ValueError):
            pm.coordinate_element_table(*bad)
    with pytest.raises(ValueError):
        pm.BoxPartition((2, 2, 2), geom_degree=5)


@pytest.mark.parametrize("kwargs", [dict(), dict(warp=twist), dict(proc_dims=(1, 1, 2), rank=1, warp=twist),
                                    dict(warp=twist, cell_frames=np.arange(48).reshape(4, 3, 4))])
def test_degree_one_partition_is_unchanged(built, kwargs):
    import pmg_dolfinx_amd as pm

    a, b = pm.BoxPartition((4, 3, 4), **kwargs), pm.BoxPartition((4, 3, 4), geom_degree=1, **kwargs)
    assert a.geom_degree == 1
    assert np.array_equal(a.xgeom, b.xgeom) and np.array_equal(a.geom_dofmap, b.geom_dofmap)
    assert a.geom_dofmap.shape == (a.ncells, 8) and a.geom_dofmap.dtype == np.int32
    for P in (1, 3):
        assert np.array_equal(a.dof_coordinates(P), b.dof_coordinates(P))
    # ... and equal to the arrays the oracle's mesh makes on one rank without frames
    if not kwargs or list(kwargs) == ["warp"]:
        from oracle import pmg_oracle as po

        m = po.BoxMesh((4, 3, 4), warp=kwargs.get("warp"))
        assert np.array_equal(a.xgeom, m.xgeom) and np.array_equal(a.geom_dofmap, m.geom_dofmap)


@pytest.mark.parametrize("g", [2, 3, 4])
def test_degree_g_partition(built, g):
    import pmg_dolfinx_amd as pm

    n = (2, 3, 2)
    part = pm.BoxPartition(n, warp=cg.quarter_annulus, geom_degree=g)
    m = g + 1
    assert part.geom_dofmap.shape == (part.ncells, m**3) and part.geom_dofmap.dtype == np.int32
    # shared nodes stored once: every node is used, no two nodes coincide
    assert part.xgeom.shape == ((2 * g + 1) * (3 * g + 1) * (2 * g + 1), 3)
    assert np.array_equal(np.unique(part.geom_dofmap), np.arange(part.xgeom.shape[0]))
    assert np.unique(np.round(part.xgeom, 12), axis=0).shape[0] == part.xgeom.shape[0]
    # the same arrays as the reference's mesh (cells lexicographic on one rank)
    x, gd = cg.box_mesh(n, g, warp=cg.quarter_annulus)
    assert np.abs(part.xgeom - x).max() < 1e-15 and np.array_equal(part.geom_dofmap, gd)
    # the corners are the degree-1 partition's vertices
    p1 = pm.BoxPartition(n, warp=cg.quarter_annulus)
    assert np.abs(part.xgeom[part.geom_dofmap[:, cg.corners(g)]] - p1.xgeom[p1.geom_dofmap]).max() < 1e-15
    # dof coordinates: the degree-g map, not the warp itself -- at P = g the dofs are the geometry nodes
    c = part.dof_coordinates(g)
    assert np.abs(c[part.level(g).dofmap] - part.xgeom[part.geom_dofmap]).max() < 1e-14
    c4 = part.dof_coordinates(4)
    box = pm.BoxPartition(n).dof_coordinates(4)
    away = np.abs(c4 - cg.quarter_annulus(box)).max()
    assert (away < 1e-14) if g == 4 else (1e-7 < away < 1e-2)
    # facet points follow the dof coordinates
    fc, fl = part.exterior_facets()
    pts = part.facet_point_coordinates(3, fc, fl)
    dm3, c3 = part.level(3).dofmap, part.dof_coordinates(3)
    assert np.array_equal(pts[5], c3[dm3[fc[5]][cg.facet_nodes(3, int(fl[5]))]])


@pytest.mark.parametrize("g", [2, 3])
def test_two_ranks_agree_on_shared_cells(built, g):
    import pmg_dolfinx_amd as pm

    n, dims = (4, 2, 2), (2, 1, 1)
    frames = np.random.default_rng(5).integers(0, 48, n)
    parts = [pm.BoxPartition(n, dims, r, warp=cg.quarter_annulus, geom_degree=g, cell_frames=frames) for r in (0, 1)]
    whole = pm.BoxPartition(n, warp=cg.quarter_annulus, geom_degree=g, cell_frames=frames)
    key = {tuple(c): i for i, c in enumerate(whole.cell_coords)}
    shared = 0
    for p in parts:
        assert p.ncells > p.ncells_owned  # a ghost layer
        for i, c in enumerate(p.cell_coords):
            want = whole.xgeom[whole.geom_dofmap[key[tuple(c)]]]
            assert np.array_equal(p.xgeom[p.geom_dofmap[i]], want)
        shared += p.ncells - p.ncells_owned
    assert shared > 0
    both = set(map(tuple, parts[0].cell_coords)) & set(map(tuple, parts[1].cell_coords))
    assert len(both) == shared


def test_reframed_geometry_rows(built):
    """``cell_frames`` lists the (g+1)^3 geometry nodes in the cell's own frame: the map of the re-framed row is the
    map of the old row with the reference coordinates permuted and reversed."""
    import pmg_dolfinx_amd as pm

    g, n = 3, (4, 3, 4)
    frames = np.random.default_rng(48).permutation(48).reshape(n)
    p0 = pm.BoxPartition(n, warp=cg.triquadratic, geom_degree=g)
    p1 = pm.BoxPartition(n, warp=cg.triquadratic, geom_degree=g, cell_frames=frames)
    assert np.array_equal(p0.xgeom, p1.xgeom)
    syms = pm.cell_symmetries()
    for c in range(p0.ncells):
        perm, flips, _ = syms[p1.cell_frames[c]]
        assert np.array_equal(p1.geom_dofmap[c], p0.geom_dofmap[c][pm.frame_node_map(g, perm, flips)])
    # the same 64-term sums in another order: 64 eps times sum |x_k| |phi_k| <= 1.2 * 2 (coordinates, Lebesgue)
    for P in (2, 4):
        assert np.abs(p1.dof_coordinates(P) - p0.dof_coordinates(P)).max() < 64 * 2.2e-16 * 2.4
