"""The Robin boundary term without a GPU: the entry points are declared, exported and bound, and the formula itself
-- d_R[dof] = sum of w1[i] w1[j] |dS| alpha over the facet points on the dof, added to the diagonal of the operator --
is pinned from first principles on the CPU oracle: the dense solve of two manufactured problems on the unit box
(Dirichlet on x = 0 and Robin elsewhere; Robin on every face and no Dirichlet dof at all) reproduces a polynomial
solution at the nodes, and without the diagonal it does not."""
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

import boundary_data_reference as bd  # noqa: E402
import robin_reference as rb  # noqa: E402

NAMES = ("pmg_laplacian_set_robin", "pmg_laplacian_has_robin")
CASES = [(1, (3, 3, 3)), (2, (3, 3, 3)), (3, (2, 3, 2)), (4, (2, 2, 2))]


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_laplacian_set_robin\(pmg_laplacian op, int32_t nfacets, const int32_t\* facet_cells,"
                     r"\s*const int8_t\* facet_local, const double\* alpha, pmg_stream \w+\);", code)
    assert re.search(r"int\s+pmg_laplacian_has_robin\(pmg_laplacian op\);", code)
    # the header says where the Robin data g goes
    assert re.search(r"pmg_laplacian_assemble_neumann with h = g", src)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is refused with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_has_robin(None) == -1
    assert lib.pmg_laplacian_has_reaction(None) == -1
    assert lib.pmg_laplacian_set_robin(None, 0, None, None, None, None) == -1
    assert b"pmg_laplacian_set_robin" in lib.pmg_last_error()


def test_python_and_cpp_layers_carry_them(built):
    import pmg_dolfinx_amd as pm

    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(pm.MatFreeLaplacian.set_robin) == ["self", "cells", "local_facets", "alpha"]
    assert sig(pm.MatFreeLaplacian.has_robin) == ["self"]
    p = inspect.signature(pm.PoissonHierarchy.__init__).parameters
    assert "robin" in p and p["robin"].default is None
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert re.search(r"void set_robin\(std::span<const std::int32_t> cells, std::span<const std::int8_t> local_facets,"
                     r"\s*std::span<const T> alpha\)", hpp)
    assert "bool has_robin() const" in hpp
    common = open(os.path.join(ROOT, "examples", "common", "rotating_tensor.hpp")).read()
    assert "linear_robin(" in common
    for driver in ("pmg", "mat_free"):
        assert '"--robin"' in open(os.path.join(ROOT, "examples", driver, driver + "_main.cpp")).read()


def test_facet_point_coordinates_follow_the_facet_nodes():
    import pmg_dolfinx_amd as pm

    P = 3
    part = pm.BoxPartition((2, 3, 2), warp=bd.twist)
    cells, facets = part.exterior_facets()
    pts = part.facet_point_coordinates(P, cells, facets)
    coords, dm = part.dof_coordinates(P), part.level(P).dofmap
    assert pts.shape == (cells.size, (P + 1) ** 2, 3)
    for F, (c, f) in enumerate(zip(cells, facets)):
        assert np.array_equal(pts[F], coords[dm[c][bd.facet_nodes_axes(P, int(f))[0]]])
    assert part.facet_point_coordinates(P, cells[:0], facets[:0]).shape == (0, (P + 1) ** 2, 3)


# ---- the formula, from first principles on the CPU oracle -----------------------------------------------------------


@pytest.mark.parametrize("dirichlet", [True, False], ids=["dirichlet-on-x0", "no-dirichlet-dof"])
@pytest.mark.parametrize("P,n", CASES)
def test_manufactured_problem_is_solved_exactly_on_the_cpu(P, n, dirichlet):
    """The load is g = kappa grad u . n + alpha u per facet point through the Neumann reference, the operator the
    dense stiffness matrix plus the face-mass diagonal: u at the nodes to rounding (measured at most 4.8e-15 with the
    marker on x = 0 and 3.7e-15 without any marked dof, when the issue was written; the bound is the boundary-data
    test's 1e-12).  Without the diagonal the same right-hand side gives another answer, or a singular matrix."""
    import pmg_dolfinx_amd as pm

    part = pm.BoxPartition(n)
    face_alpha = rb.FACE_ALPHA if dirichlet else rb.FACE_ALPHA_NO_DIRICHLET
    u, b, d_R, marker, K = rb.manufactured_problem(part, P, face_alpha, dirichlet)
    assert bool(marker.any()) == dirichlet
    x, M = rb.dense_solve(u, b, d_R, marker, K)
    err = np.abs(x - u).max() / np.abs(u).max()
    free = ~marker.astype(bool)
    lam = np.linalg.eigvalsh(M[np.ix_(free, free)])[0]
    print(f"P = {P}, cells {n}, {'Dirichlet on x = 0' if dirichlet else 'no Dirichlet dof'}: "
          f"max|x - u| / max|u| = {err:.2e}, smallest eigenvalue {lam:.3e}")
    assert err < 1e-12
    assert lam > 1e-3  # well posed, also without a Dirichlet dof
    lam0 = np.linalg.eigvalsh(K[np.ix_(free, free)])[0]
    if dirichlet:
        x0, _ = rb.dense_solve(u, b, np.zeros_like(d_R), marker, K)
        away = np.abs(x0 - u).max() / np.abs(u).max()
        print(f"    without the diagonal: {away:.2e} away")
        assert away > 1e-2
    else:
        assert abs(lam0) < 1e-12 * np.abs(K).max()  # the pure Neumann operator: singular


def test_robin_vector_sums_to_alpha_times_area():
    """A per-face constant alpha on the unit box: sum(d_R) = sum_faces alpha_face * 1.  On the twisted box a dof on
    an edge between two faces carries both faces' weights (the reason alpha is per facet point, not per dof)."""
    import pmg_dolfinx_amd as pm

    P = 3
    nf = (P + 1) ** 2
    part = pm.BoxPartition((2, 2, 2))
    lv = part.level(P)
    cells, facets = part.exterior_facets()
    nomark = np.zeros(lv.ndofs, dtype=np.int8)
    alpha = np.repeat(np.asarray(rb.FACE_ALPHA_NO_DIRICHLET)[facets.astype(int)][:, None], nf, axis=1)
    d = rb.robin_vector(part, P, lv.dofmap, cells, facets, alpha, nomark)
    assert abs(d.sum() - sum(rb.FACE_ALPHA_NO_DIRICHLET)) < 1e-13
    assert np.all(d[~lv.bc_marker.astype(bool)] == 0.0)  # interior dofs carry none
    # marked dofs carry none
    marker = rb.one_face_marker(lv.bc_marker, part.dof_coordinates(P))
    dm = rb.robin_vector(part, P, lv.dofmap, cells, facets, alpha, marker)
    assert np.all(dm[marker.astype(bool)] == 0.0) and np.array_equal(dm[~marker.astype(bool)], d[~marker.astype(bool)])
    # twisted box: per face, then the edge dofs
    tw = pm.BoxPartition((2, 2, 2), warp=bd.twist)
    per_face = []
    for f in range(6):
        on = facets == f
        per_face.append(rb.robin_vector(tw, P, lv.dofmap, cells[on], facets[on], alpha[on], nomark))
    both = rb.robin_vector(tw, P, lv.dofmap, cells, facets, alpha, nomark)
    assert np.abs(both - np.sum(per_face, axis=0)).max() < 1e-15
    edge = (per_face[2] > 0) & (per_face[4] > 0)  # dofs on the edge y = 0, z = 0
    assert edge.sum() == 2 * P + 1
    assert np.all(both[edge] > np.maximum(per_face[2], per_face[4])[edge])
    wds, _ = bd.facet_geometry(tw, P, cells, facets)
    assert abs(both.sum() - (wds * alpha).sum()) < 1e-13


def test_reference_wrapper_adds_both_diagonals():
    import pmg_dolfinx_amd as pm
    import reaction_reference as rr

    P = 2
    part = pm.BoxPartition((2, 3, 2), warp=bd.twist)
    lv = part.level(P)
    cells, facets = part.exterior_facets()
    marker = rb.one_face_marker(lv.bc_marker, part.dof_coordinates(P))
    alpha = rb.random_alpha(cells.size, (P + 1) ** 2, 1)
    assert 0.1 < (alpha == 0).mean() < 0.3 and alpha.max() <= 4.0
    sigma = rr.random_sigma(part.ncells, 2)
    A = rb.laplacian(part, P, 0.3, lv.dofmap, marker, cells, facets, alpha, sigma)
    u = np.random.default_rng(3).standard_normal(lv.ndofs)
    want = A.A.apply(u) + (rr.reaction_vector(P, sigma, lv.dofmap, part.xgeom, part.geom_dofmap, marker)
                           + rb.robin_vector(part, P, lv.dofmap, cells, facets, alpha, marker)) * u
    assert np.array_equal(A.apply(u), want)
    assert np.array_equal(A.apply(u)[marker.astype(bool)], u[marker.astype(bool)])
    assert np.abs(A.dense() @ u - A.apply(u)).max() < 1e-12 * np.abs(u).max()
    assert np.array_equal(A.diagonal(), A.A.diagonal() + A.d)
