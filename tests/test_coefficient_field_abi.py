"""The nodal coefficient field without a GPU: the two entry points are declared, exported and bound, the Python
layers carry them, and the CPU truth every GPU test of tests/test_gpu_coefficient_field.py compares against -- the
oracle's operator with its stored tensor scaled point by point -- is the stiffness matrix of
-div(kappa kq grad u) assembled from first principles."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from oracle import pmg_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("pmg_laplacian_set_coefficient_field", "pmg_laplacian_has_coefficient_field")


def _declared():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", src))


def test_header_declares_the_entry_points():
    declared = _declared()
    for name in NAMES:
        assert name in declared
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    assert re.search(r"int\s+pmg_laplacian_set_coefficient_field\(pmg_laplacian op, const double\* kq, "
                     r"pmg_stream stream\);", src)
    assert re.search(r"int\s+pmg_laplacian_has_coefficient_field\(pmg_laplacian op\);", src)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is an error with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_has_coefficient_field(None) == -1
    assert lib.pmg_laplacian_set_coefficient_field(None, None, None) == -1
    assert b"pmg_laplacian_set_coefficient_field" in lib.pmg_last_error()


def test_python_layers_carry_the_field(built):
    import pmg_dolfinx_amd as pm

    for method in ("set_coefficient_field", "has_coefficient_field"):
        assert callable(getattr(pm.MatFreeLaplacian, method))
    assert list(inspect.signature(pm.MatFreeLaplacian.set_coefficient_field).parameters) == ["self", "v"]
    p = inspect.signature(pm.PoissonHierarchy.__init__).parameters
    assert "kappa_field" in p and p["kappa_field"].default is None
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "void set_coefficient_field(const Vector& kq)" in hpp and "void clear_coefficient_field()" in hpp


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def _dense_first_principles(mesh, P, kappa, kq):
    """K[i, j] = sum_cells sum_q w_q |det J_q| kappa_c kq[dof(c, q)] grad phi_i(x_q) . grad phi_j(x_q): the GLL-collocated
    stiffness matrix written down from the weak form (physical gradients J^-T grad_ref, no adjugate, no stored
    tensor), without boundary conditions."""
    nd = P + 1
    xi, w = po.gll_points_weights(nd)
    L = po.lagrange_eval_matrix(xi, xi)    # [point, basis] = identity
    D = po.lagrange_deriv_matrix(xi)       # [point, basis]
    # reference gradients of the nd^3 basis functions at the nd^3 points: [3, q, i], q and i as a*nd^2 + b*nd + c
    gr = np.stack([np.einsum("ai,bj,ck->abcijk", D, L, L), np.einsum("ai,bj,ck->abcijk", L, D, L),
                   np.einsum("ai,bj,ck->abcijk", L, L, D)]).reshape(3, nd**3, nd**3)
    w3 = np.einsum("a,b,c->abc", w, w, w).ravel()
    phi, dph = np.stack([1.0 - xi, xi], axis=1), np.stack([-np.ones(nd), np.ones(nd)], axis=1)
    dN = np.stack([np.einsum("ai,bj,cl->abcijl", dph, phi, phi), np.einsum("ai,bj,cl->abcijl", phi, dph, phi),
                   np.einsum("ai,bj,cl->abcijl", phi, phi, dph)]).reshape(3, nd**3, 8)  # vertex k = i*4 + j*2 + l
    dofmap = mesh.dofmap(P)
    n = mesh.ndofs(P)
    K = np.zeros((n, n))
    for c in range(mesh.ncells):
        xc = mesh.xgeom[mesh.geom_dofmap[c]]  # [8, 3]
        dofs = dofmap[c]
        for q in range(nd**3):
            J = np.einsum("kd,rk->dr", xc, dN[:, q, :])  # J[d, r] = d x_d / d xi_r
            g = np.linalg.solve(J.T, gr[:, q, :])        # physical gradients [3, i]
            K[np.ix_(dofs, dofs)] += w3[q] * abs(np.linalg.det(J)) * kappa[c] * kq[dofs[q]] * (g.T @ g)
    return K


def test_scaled_oracle_is_the_variable_coefficient_operator():
    P = 2
    mesh = po.BoxMesh((2, 2, 2), warp=twist)
    rng = np.random.default_rng(0)
    kappa = rng.uniform(1.0, 3.0, mesh.ncells)
    kq = rng.uniform(0.5, 2.0, mesh.ndofs(P))
    nobc = np.zeros(mesh.ndofs(P), dtype=np.int8)
    A = po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc)
    plain = A.assemble_csr().toarray()
    A.G *= kq[A.dofmap][:, :, None]
    A._diag = None
    M = A.assemble_csr().toarray()
    K = _dense_first_principles(mesh, P, kappa, kq)
    scale = np.abs(K).max()
    assert np.abs(M - K).max() < 1e-12 * scale
    assert np.abs(plain - K).max() > 1e-2 * scale  # the field is seen
    # symmetric, positive semi-definite with the constants as its only null space
    assert np.abs(M - M.T).max() < 1e-13 * scale
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert abs(ev[0]) < 1e-11 * ev[-1] and ev[1] > 1e-6 * ev[-1]
    # apply and diagonal of the scaled oracle are those of that matrix
    u = rng.standard_normal(mesh.ndofs(P))
    assert np.abs(A.apply(u) - K @ u).max() < 1e-12 * np.abs(K @ u).max()
    assert np.abs(A.diagonal() - np.diag(K)).max() < 1e-12 * np.diag(K).max()
    # with Dirichlet rows it is symmetric positive definite
    bc = mesh.boundary_marker(P)
    B = po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, bc)
    B.G *= kq[B.dofmap][:, :, None]
    B._diag = None
    Mb = B.assemble_csr().toarray()
    free = ~bc.astype(bool)
    assert np.abs(Mb[np.ix_(free, free)] - K[np.ix_(free, free)]).max() < 1e-12 * scale
    assert np.array_equal(Mb[~free][:, ~free], np.eye(int((~free).sum())))
    assert np.abs(Mb - Mb.T).max() < 1e-13 * scale and np.linalg.eigvalsh(0.5 * (Mb + Mb.T)).min() > 0
