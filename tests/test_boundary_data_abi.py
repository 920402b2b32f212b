"""Boundary data without a GPU: the entry points are declared, exported and bound; the facet helpers of mesh.py
number faces and face points as include/pmg_amd.h says; and the method itself -- lifting with the unconstrained
operator, the GLL-collocated Neumann load with |dS| = |row `axis` of adj(J)|, the facet numbering 2 * axis + side -- is
pinned from first principles on the CPU oracle: the dense solve of a mixed Dirichlet / Neumann problem reproduces a
polynomial solution at the nodes."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as ref  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

NAMES = ("pmg_laplacian_apply_lifting", "pmg_laplacian_set_bc", "pmg_laplacian_assemble_neumann")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_laplacian_apply_lifting\(pmg_laplacian op, double\* g, const double\* x0, "
                     r"double alpha, double\* b,\s*pmg_stream \w+\);", code)
    assert re.search(r"int\s+pmg_laplacian_set_bc\(pmg_laplacian op, const double\* g, const double\* x0, "
                     r"double alpha, double\* b,\s*pmg_stream \w+\);", code)
    assert re.search(r"int\s+pmg_laplacian_assemble_neumann\(pmg_laplacian op, int32_t nfacets, "
                     r"const int32_t\* facet_cells,\s*const int8_t\* facet_local, const double\* h, double\* b, "
                     r"pmg_stream \w+\);", code)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is PMG_ERR_INVALID with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_apply_lifting(None, None, None, 1.0, None, None) == -1
    assert b"pmg_laplacian_apply_lifting" in lib.pmg_last_error()
    assert lib.pmg_laplacian_set_bc(None, None, None, 1.0, None, None) == -1
    assert b"pmg_laplacian_set_bc" in lib.pmg_last_error()
    assert lib.pmg_laplacian_assemble_neumann(None, 0, None, None, None, None, None) == -1
    assert b"pmg_laplacian_assemble_neumann" in lib.pmg_last_error()


def test_python_and_cpp_layers_carry_them(built):
    import pmg_dolfinx_amd as pm

    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(pm.MatFreeLaplacian.apply_lifting) == ["self", "g", "b", "x0", "alpha"]
    assert sig(pm.MatFreeLaplacian.set_bc) == ["self", "g", "b", "x0", "alpha"]
    assert sig(pm.MatFreeLaplacian.assemble_neumann) == ["self", "cells", "local_facets", "h", "b"]
    p = inspect.signature(pm.MatFreeLaplacian.apply_lifting).parameters
    assert p["x0"].default is None and p["alpha"].default == 1.0
    assert callable(pm.facet_nodes) and callable(pm.BoxPartition.exterior_facets)
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    for text in ("void apply_lifting(Vector& g, Vector& b, T alpha = 1)",
                 "void apply_lifting(Vector& g, const Vector& x0, Vector& b, T alpha = 1)",
                 "void set_bc(const Vector& g, Vector& b, T alpha = 1)", "void assemble_neumann("):
        assert text in hpp, text
    common = open(os.path.join(ROOT, "examples", "common", "box_mesh.hpp")).read()
    assert "facet_nodes(int P, int local_facet)" in common and "exterior_facets(" in common


# ---- the facet helpers, pure numpy ----------------------------------------------------------------------------------


def test_exterior_facets_of_a_box():
    import pmg_dolfinx_amd as pm

    n = (2, 3, 4)
    part = pm.BoxPartition(n)
    cells, facets = part.exterior_facets()
    assert cells.dtype == np.int32 and facets.dtype == np.int8
    assert cells.size == facets.size == 2 * (2 * 3 + 3 * 4 + 2 * 4)
    assert len(set(zip(cells.tolist(), facets.tolist()))) == cells.size  # each (cell, facet) once
    assert cells.min() >= 0 and cells.max() < part.ncells and facets.min() >= 0 and facets.max() <= 5
    # all nodes of each listed face lie on the matching boundary plane
    P = 3
    coords, dm = part.dof_coordinates(P), part.level(P).dofmap
    for c, f in zip(cells, facets):
        axis, side = int(f) // 2, int(f) % 2
        x = coords[dm[c][pm.facet_nodes(P, int(f))]]
        assert np.abs(x[:, axis] - float(side)).max() < 1e-14, (c, f)
    # every one of the six planes is there with its own number of faces
    for f, count in zip(range(6), (12, 12, 8, 8, 6, 6)):
        assert int((facets == f).sum()) == count


def test_exterior_facets_of_two_bricks_include_the_ghost_cells():
    import pmg_dolfinx_amd as pm

    n = (2, 2, 4)
    for rank in (0, 1):
        part = pm.BoxPartition(n, (1, 1, 2), rank)
        cells, facets = part.exterior_facets()
        assert part.ncells > part.ncells_owned and (cells >= part.ncells_owned).any()
        cc = part.cell_coords[cells]
        for c, f in zip(cc, facets):
            axis, side = int(f) // 2, int(f) % 2
            assert c[axis] == (n[axis] - 1 if side else 0)
        # nothing is missing: every local cell on a boundary plane is listed for it
        expect = sum(int((part.cell_coords[:, a] == v).sum()) for a in range(3) for v in (0, n[a] - 1))
        assert cells.size == expect


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_facet_nodes(P):
    import pmg_dolfinx_amd as pm

    nd = P + 1
    for f in range(6):
        t = pm.facet_nodes(P, f)
        axis, side = f // 2, f % 2
        assert t.shape == (nd * nd,) and len(set(t.tolist())) == nd * nd
        abc = np.stack([t // (nd * nd), (t // nd) % nd, t % nd], axis=1)
        assert np.all(abc[:, axis] == (P if side else 0))
        # s = i * nd + j over the two remaining axes in increasing axis order, ascending
        rest = [a for a in range(3) if a != axis]
        s = np.arange(nd * nd)
        assert np.array_equal(abc[:, rest[0]], s // nd) and np.array_equal(abc[:, rest[1]], s % nd)
        assert np.array_equal(t, ref.facet_nodes_axes(P, f)[0])
    with pytest.raises(ValueError):
        pm.facet_nodes(P, 6)


# ---- the method, from first principles on the CPU oracle -------------------------------------------------------------


def _unconstrained_dense(P, part, lv):
    A = po.Laplacian(P, ref.KAPPA, lv.dofmap, part.xgeom, part.geom_dofmap, np.zeros(lv.ndofs, dtype=np.int8))
    Ae = A.element_matrices()
    K = np.zeros((lv.ndofs, lv.ndofs))
    for c in range(part.ncells):
        K[np.ix_(A.dofmap[c], A.dofmap[c])] += Ae[c]
    return A, K


@pytest.mark.parametrize("P,n", [(2, (3, 3, 3)), (3, (2, 3, 2)), (4, (2, 2, 2))])
def test_mixed_problem_is_solved_exactly_on_the_cpu(P, n):
    """Lifting + Neumann load + volume load, dense solve: u at the nodes to rounding (measured 6e-16, 9e-16, 1.3e-15
    when the issue was written; bound 1e-12).  Pins |dS| = |row axis of adj(J)| and the facet numbering."""
    import pmg_dolfinx_amd as pm

    part = pm.BoxPartition(n)
    lv = part.level(P)
    cells, facets = part.exterior_facets()
    u, f_over_kappa, h, marker = ref.mixed_problem_data(part, P, cells, facets)
    A, K = _unconstrained_dense(P, part, lv)
    marked = marker.astype(bool)
    assert marked.any() and (lv.bc_marker.astype(bool) & ~marked).any()  # both kinds of boundary are there
    # volume load with the oracle's detJ and weights: b_i = sum_cells kappa w_q detJ_q (f / kappa)_i
    b = np.bincount(A.dofmap.ravel(), weights=(ref.KAPPA * A.w3[None, :] * A.detJ * f_over_kappa[A.dofmap]).ravel(),
                    minlength=lv.ndofs)
    b += ref.neumann_reference(part, P, lv.dofmap, cells, facets, h, np.zeros_like(marker), lv.ndofs)
    g = np.where(marked, u, 0.0)
    b -= K @ g  # apply_lifting
    free = ~marked
    x = u.copy()
    x[free] = np.linalg.solve(K[np.ix_(free, free)], b[free])
    err = np.abs(x - u).max() / np.abs(u).max()
    print(f"P = {P}, cells {n}: max|x - u| / max|u| = {err:.2e}")
    assert err < 1e-12
    # the wrong sign of the normal, or the neighbouring axis, is seen at once
    wrong = ref.neumann_reference(part, P, lv.dofmap, cells, facets ^ 1, h, np.zeros_like(marker), lv.ndofs)
    assert np.abs(wrong - ref.neumann_reference(part, P, lv.dofmap, cells, facets, h, np.zeros_like(marker),
                                                lv.ndofs)).max() > 1e-3


def test_surface_element_sums_to_the_area_of_a_warped_box_face():
    """sum of w2 |dS| over the faces of the unit box is 6 (exactly integrable), and on the twisted box every
    shared-edge dof gets both faces' contributions with their own normals (the reason h is per facet point)."""
    import pmg_dolfinx_amd as pm

    P = 3
    part = pm.BoxPartition((2, 2, 2))
    cells, facets = part.exterior_facets()
    wds, normal = ref.facet_geometry(part, P, cells, facets)
    assert abs(wds.sum() - 6.0) < 1e-13
    for f in range(6):
        want = np.zeros(3)
        want[f // 2] = 1.0 if f % 2 else -1.0
        assert np.abs(normal[facets == f] - want).max() < 1e-14
    tw = pm.BoxPartition((2, 2, 2), warp=ref.twist)
    wds_t, normal_t = ref.facet_geometry(tw, P, cells, facets)
    assert np.abs(np.linalg.norm(normal_t, axis=2) - 1.0).max() < 1e-14 and wds_t.min() > 0
    # outward: the normal points away from the cell's centroid
    lv = tw.level(P)
    coords = tw.dof_coordinates(P)
    for F, (c, lf) in enumerate(zip(cells, facets)):
        centre = tw.xgeom[tw.geom_dofmap[c]].mean(axis=0)
        pts = coords[lv.dofmap[c][ref.facet_nodes_axes(P, int(lf))[0]]]
        assert (np.einsum("sd,sd->s", pts - centre, normal_t[F]) > 0).all()
