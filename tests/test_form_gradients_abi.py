"""The coefficient gradients of the form (pmg_laplacian_form_gradients) without a GPU: the interface is there at every
layer, and the numpy reference the GPU tests compare with (tests/form_gradients_reference.py, written from the weak
form) is the derivative of the oracle's operator in each coefficient and satisfies the Euler identities.

Bars.  A is linear in each coefficient, so a difference quotient with an O(1) step is exact to rounding; its bar is the
one of tests/test_cell_form_abi.py, 1e-12 (|v_m| . |y0| + |v_m| . |y1|) / delta: the two products are what rounds.  The
Euler identities hold to 1e-12 of the summed scales of the reference's terms."""
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

import curved_geometry_reference as cr  # noqa: E402
import form_gradients_reference as fg  # noqa: E402
import reaction_reference as rr  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

NAME = "pmg_laplacian_form_gradients"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the interface, layer by layer --------------------------------------------------------------------------------


def test_header_declares_the_entry_point():
    h = _read("include", "pmg_amd.h")
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, "the header does not declare " + NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[0].startswith("pmg_laplacian") and args[-1].startswith("pmg_stream")
    assert args[1].startswith("const double*") and args[2].startswith("const double*")
    assert [a.split()[-1] for a in args[3:7]] == ["d_kappa", "d_field", "d_tensor", "d_sigma"]
    assert all(a.startswith("double*") for a in args[3:7]) and args[7].startswith("int")
    # the paragraph comes after the cell form's, and says what the caller has to know
    assert h.index("coefficient gradients of the form") > h.index("#define PMG_CELL_FORM_CONSTRAINED")
    doc = re.sub(r"\s*\n \*\s*", " ", h[h.index("coefficient gradients of the form"):h.index("int " + NAME)])
    assert "NO EXCHANGE" in doc and "not collective" in doc and "NOT zero on marked dofs" in doc


def test_library_exports_and_binding_covers_it(built):
    import pmg_dolfinx_amd as pm

    assert hasattr(pm._lib.lib(), NAME)
    res, args = pm._lib._SIGS[NAME]
    assert res is C.c_int and len(args) == 9 and args[7] is C.c_int


def test_null_handle_is_refused_by_name(built):
    import pmg_dolfinx_amd as pm

    L = pm._lib.lib()
    assert L.pmg_laplacian_form_gradients(None, None, None, None, None, None, None, 0, None) == -1
    assert NAME in L.pmg_last_error().decode()


def test_python_cpp_and_driver_carry_it(built):
    import pmg_dolfinx_amd as pm

    sig = inspect.signature(pm.MatFreeLaplacian.form_gradients)
    assert list(sig.parameters)[1:] == ["u", "v", "kappa", "field", "tensor", "sigma", "constrained", "out"]
    assert [sig.parameters[k].default for k in ("kappa", "field", "tensor", "sigma", "constrained", "out")] \
        == [False, False, False, False, True, None]
    sig = inspect.signature(pm.adjoint.solve)
    assert list(sig.parameters) == ["op", "cg", "b", "kappa", "preconditioner", "field", "tensor", "sigma"]
    for k in ("field", "tensor", "sigma"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is None
    hpp = _read("include", "pmg_amd.hpp")
    assert re.search(r"void\s+form_gradients\s*\(\s*const Vector&\s*u,\s*const Vector&\s*v,", hpp) and NAME in hpp
    drv = _read("examples", "mat_free", "mat_free_main.cpp")
    assert '"--form-gradients"' in drv and "op.form_gradients(" in drv


# ---- the reference ------------------------------------------------------------------------------------------------


class Case:
    """The jittered (3, 2, 2) box with one Dirichlet face and every coefficient set, and the oracle's operator of it."""

    def __init__(self, P, seed=0):
        self.P = P
        self.mesh = mesh = po.BoxMesh((3, 2, 2), warp=fg.jitter)
        self.dm = mesh.dofmap(P)
        marker = np.zeros(mesh.dof_shape(P), dtype=np.int8)
        marker[0, :, :] = 1
        self.marker = marker.ravel()
        rng = np.random.default_rng(100 * P + seed)
        n = mesh.ndofs(P)
        self.kappa = rng.uniform(1.0, 2.0, mesh.ncells)
        self.kq = rng.uniform(0.5, 2.0, n)
        self.T = tr.random_spd(mesh.ncells, 7 + seed)
        self.sigma = rng.uniform(0.0, 3.0, mesh.ncells)
        self.u, self.v = rng.standard_normal(n), rng.standard_normal(n)
        self.vm = np.where(self.marker.astype(bool), 0.0, self.v)

    def diffusion(self, kappa=None, kq=None, T=None):
        A = cr.laplacian(self.P, 1, self.kappa if kappa is None else kappa, self.dm, self.mesh.xgeom,
                         self.mesh.geom_dofmap, self.marker)
        return cr.with_tensor(A, self.T if T is None else T, self.kq if kq is None else kq)

    def apply(self, sigma=None, **kw):
        A = rr.ReactionLaplacian(self.diffusion(**kw), self.sigma if sigma is None else sigma, self.mesh.xgeom,
                                 self.mesh.geom_dofmap)
        return A.apply(self.u)

    def reference(self, marker=True):
        return fg.form_gradients(self.P, self.dm, self.mesh.xgeom, self.mesh.geom_dofmap, self.u, self.v, self.kappa,
                                 marker=self.marker if marker else None, kq=self.kq, T=self.T,
                                 ndofs=self.mesh.ndofs(self.P))

    def dofs(self):
        """An interior dof, a dof shared across a face, a marked dof."""
        nd = self.P + 1
        dm = self.dm.reshape(-1, nd, nd, nd)
        count = np.bincount(self.dm.ravel(), minlength=self.marker.size)
        free = ~self.marker.astype(bool)
        inner, shared = int(dm[0, 1, 1, 1]), int(dm[0, nd - 1, 1, 1])  # inside cell 0, inside its face to the next cell
        if self.P == 1:  # vertices: inside the box, inside a face of the box
            shared = int(np.flatnonzero((count == 4) & free)[0])
        assert (count[inner], count[shared]) == ((1, 2) if self.P >= 2 else (8, 4)) and free[inner] and free[shared]
        marked = int(np.flatnonzero(self.marker)[3])
        return inner, shared, marked


def spd(T):
    xx, xy, xz, yy, yz, zz = np.asarray(T).T
    det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz)
    return bool(np.all(xx > 0) and np.all(xx * yy - xy * xy > 0) and np.all(det > 0))


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_reference_is_the_exact_derivative_of_the_oracle(P):
    case = Case(P, seed=2)
    ref = case.reference()
    y0 = case.apply()

    def check(what, want, y1, delta):
        got = case.vm @ (y1 - y0) / delta
        bar = 1e-12 * (np.abs(case.vm) @ np.abs(y0) + np.abs(case.vm) @ np.abs(y1)) / abs(delta)
        print(f"P={P} {what}: diff / bar = {abs(got - want) / bar:.3e}")
        assert abs(got - want) <= bar, (what, got, want, bar)

    delta = 0.75
    for c in (0, 5, 11):
        k1 = case.kappa.copy()
        k1[c] += delta
        check(f"kappa[{c}]", ref["kappa"][0][c], case.apply(kappa=k1), delta)
        s1 = case.sigma.copy()
        s1[c] += delta
        check(f"sigma[{c}]", ref["sigma"][0][c], case.apply(sigma=s1), delta)
    for n in case.dofs():
        q1 = case.kq.copy()
        q1[n] += delta
        check(f"field[{n}]", ref["field"][0][n], case.apply(kq=q1), delta)
    assert ref["field"][0][case.dofs()[2]] != 0.0  # not zero on a marked dof
    # tensor steps that keep the leading minors positive: any step up a diagonal entry does; the eigenvalues are at
    # least 0.5 (random_spd), so an off-diagonal step of 0.25, a perturbation of norm 0.25, does too
    for c, k, d in ((0, 0, 0.75), (5, 3, 0.75), (11, 5, 0.75), (0, 1, 0.25), (5, 2, 0.25), (11, 4, -0.25)):
        T1 = case.T.copy()
        T1[c, k] += d
        assert spd(case.T) and spd(T1)
        check(f"tensor[{c}][{k}]", ref["tensor"][0][c, k], case.apply(T=T1), d)


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_euler_identities_hold_for_the_oracle(P):
    """A_diff is linear in kappa, in kq and in T: each coefficient times its gradient sums to v_m . A_diff u_m."""
    case = Case(P, seed=1)
    ref = case.reference()
    want = case.vm @ case.diffusion().apply(case.u)
    sums = {"kappa": (case.kappa @ ref["kappa"][0], case.kappa @ ref["kappa"][1]),
            "field": (case.kq @ ref["field"][0], case.kq @ ref["field"][1]),
            "tensor": ((case.T * ref["tensor"][0]).sum(), (np.abs(case.T) * ref["tensor"][1]).sum())}
    for name, (got, S) in sums.items():
        print(f"P={P} {name}: |sum - v_m . A_diff u_m| / S = {abs(got - want) / S:.3e}")
        assert abs(got - want) <= 1e-12 * S, name
    # and the reaction term's: sum_c sigma_c d_sigma[c] = v_m . (d .* u_m)
    d = rr.reaction_vector(P, case.sigma, case.dm, case.mesh.xgeom, case.mesh.geom_dofmap, case.marker)
    assert abs(case.sigma @ ref["sigma"][0] - case.vm @ (d * case.u)) <= 1e-12 * (case.sigma @ ref["sigma"][1])


def test_d_kappa_is_the_cell_form():
    import cell_form_reference as cf

    case = Case(3)
    for marker in (None, case.marker):
        e, S = cf.cell_form(3, case.dm, case.mesh.xgeom, case.mesh.geom_dofmap, case.u, case.v, marker=marker,
                            kq=case.kq, T=case.T)
        got = case.reference(marker is not None)["kappa"]
        assert np.all(np.abs(got[0] - e) <= 1e-13 * S) and np.allclose(got[1], S, rtol=1e-12)
