"""The per-cell bilinear form (pmg_laplacian_cell_form) without a GPU: the interface is there at every layer, and the
numpy reference the GPU tests compare with (tests/cell_form_reference.py, written from the weak form) agrees with the
oracle's element kernel and satisfies, for the oracle, the two identities the GPU tests check through the library.

Bars.  Reference against ``sum(ve * cell_apply(ue))``: both are float64 sums of at most 216 point terms whose factors
carry a few tens of roundings each (two 3x3 inverses or adjugates, six contractions of length <= 6), so they differ by
well under 50 eps S_c = 6e-15 S_c, S_c = sum_q |term_q|; the bar is 1e-13 S_c.  The two identities carry the bars the GPU
tests use (1e-12 of the sums of magnitudes)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cell_form_reference as cf  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

NAME = "pmg_laplacian_cell_form"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the interface, layer by layer --------------------------------------------------------------------------------


def test_header_declares_the_entry_point_and_both_flags():
    h = _read("include", "pmg_amd.h")
    assert re.search(r"^#define\s+PMG_CELL_FORM_KAPPA\s+1\b", h, re.M)
    assert re.search(r"^#define\s+PMG_CELL_FORM_CONSTRAINED\s+2\b", h, re.M)
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, "the header does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6 and args[0].startswith("pmg_laplacian") and args[-1].startswith("pmg_stream")
    assert args[1].startswith("const double*") and args[2].startswith("const double*") and args[3].startswith("double*")
    # what the caller has to know: no exchange, and which terms are in
    doc = h[h.index("per-cell bilinear form"):h.index("#define PMG_CELL_FORM_KAPPA")]
    assert "NO EXCHANGE" in doc and "not collective" in doc
    assert "reaction and Robin terms" in doc and "are not provided" in doc


def test_library_exports_and_binding_covers_it(built):
    import pmg_dolfinx_amd as pm

    assert hasattr(pm._lib.lib(), NAME)
    res, args = pm._lib._SIGS[NAME]
    assert res is C.c_int and len(args) == 6 and args[4] is C.c_int


def test_null_handle_is_refused_by_name(built):
    import pmg_dolfinx_amd as pm

    L = pm._lib.lib()
    assert L.pmg_laplacian_cell_form(None, None, None, None, 0, None) == -1
    assert NAME in L.pmg_last_error().decode()


def test_python_cpp_and_driver_carry_it(built):
    import pmg_dolfinx_amd as pm

    assert callable(getattr(pm.MatFreeLaplacian, "cell_form"))
    assert pm.MatFreeLaplacian.CELL_FORM_KAPPA == 1 and pm.MatFreeLaplacian.CELL_FORM_CONSTRAINED == 2
    assert callable(pm.adjoint.solve)
    hpp = _read("include", "pmg_amd.hpp")
    assert re.search(r"void\s+cell_form\s*\(\s*const Vector&\s*u,\s*const Vector&\s*v,\s*std::span<T>\s*out_device", hpp)
    assert NAME in hpp
    drv = _read("examples", "mat_free", "mat_free_main.cpp")
    assert '"--cell-form"' in drv and "op.cell_form(" in drv


# ---- the reference ------------------------------------------------------------------------------------------------


def _case(P, seed=0):
    mesh = po.BoxMesh((3, 2, 2), warp=cf.jitter)
    dm = mesh.dofmap(P)
    nd0 = mesh.dof_shape(P)
    marker = np.zeros(nd0, dtype=np.int8)
    marker[0, :, :] = 1  # Dirichlet on one face: marked and unmarked dofs share cells
    marker = marker.ravel()
    rng = np.random.default_rng(100 * P + seed)
    kappa = rng.uniform(1.0, 2.0, mesh.ncells)
    u, v = rng.standard_normal(mesh.ndofs(P)), rng.standard_normal(mesh.ndofs(P))
    return mesh, dm, marker, kappa, u, v


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_reference_equals_the_oracles_element_kernel(P):
    mesh, dm, marker, kappa, u, v = _case(P)
    nd = P + 1
    A = po.Laplacian(P, kappa, dm, mesh.xgeom, mesh.geom_dofmap, marker)
    ue, ve = u[dm].reshape(-1, nd, nd, nd), v[dm].reshape(-1, nd, nd, nd)
    want = (ve * A.cell_apply(ue)).reshape(mesh.ncells, -1).sum(axis=1)
    e, S = cf.cell_form(P, dm, mesh.xgeom, mesh.geom_dofmap, u, v, kappa=kappa)
    print("P", P, "max |diff| / S_c", np.abs(e - want).max() / S.max(), (np.abs(e - want) / S).max())
    assert np.all(np.abs(e - want) <= 1e-13 * S)
    # without kappa: the same divided out
    e0, S0 = cf.cell_form(P, dm, mesh.xgeom, mesh.geom_dofmap, u, v)
    assert np.all(np.abs(e0 * kappa - want) <= 1e-13 * S)
    assert np.all(S0 > 0)


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_sum_identity_holds_for_the_oracle(P):
    """sum_c e_c(u, v) with kappa and the marked dofs zeroed = v_m . A u_m."""
    mesh, dm, marker, kappa, u, v = _case(P, seed=1)
    A = po.Laplacian(P, kappa, dm, mesh.xgeom, mesh.geom_dofmap, marker)
    m = marker.astype(bool)
    um, vm = np.where(m, 0.0, u), np.where(m, 0.0, v)
    e, S = cf.cell_form(P, dm, mesh.xgeom, mesh.geom_dofmap, u, v, kappa=kappa, marker=marker)
    want = vm @ A.apply(um)
    print("P", P, "rel. to sum S_c", abs(e.sum() - want) / S.sum())
    assert abs(e.sum() - want) <= 1e-12 * S.sum()


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_exact_derivative_holds_for_the_oracle(P):
    """A is linear in kappa: v_m . (A(kappa + delta e_c) u - A(kappa) u) / delta = e_c(u, v), constrained, no kappa."""
    mesh, dm, marker, kappa, u, v = _case(P, seed=2)
    m = marker.astype(bool)
    vm = np.where(m, 0.0, v)
    e, _ = cf.cell_form(P, dm, mesh.xgeom, mesh.geom_dofmap, u, v, marker=marker)
    y0 = po.Laplacian(P, kappa, dm, mesh.xgeom, mesh.geom_dofmap, marker).apply(u)
    delta = 0.75
    for c in (0, 5, 11):
        k1 = kappa.copy()
        k1[c] += delta
        y1 = po.Laplacian(P, k1, dm, mesh.xgeom, mesh.geom_dofmap, marker).apply(u)
        got = vm @ (y1 - y0) / delta
        bar = 1e-12 * (np.abs(vm) @ np.abs(y0) + np.abs(vm) @ np.abs(y1)) / delta
        print("P", P, "cell", c, "diff / bar", abs(got - e[c]) / bar)
        assert abs(got - e[c]) <= bar
