"""The per-cell diffusion tensor without a GPU: the two entry points are declared, exported and bound, the Python and
C++ layers carry them, and the CPU truth every GPU test of tests/test_gpu_coefficient_tensor.py compares against --
the oracle's operator with its stored tensor replaced by adj(J) K adj(J)^T w / det J
(tests/tensor_coefficient_reference.py) -- is the stiffness matrix of -div(kappa K grad u) written down from the weak
form, with the components of K in the order (xx, xy, xz, yy, yz, zz)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tensor_coefficient_reference as tr  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

NAMES = ("pmg_laplacian_set_coefficient_tensor", "pmg_laplacian_has_coefficient_tensor")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", bare))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_laplacian_set_coefficient_tensor\(pmg_laplacian op, const double\* kt, "
                     r"pmg_stream stream\);", bare)
    assert re.search(r"int\s+pmg_laplacian_has_coefficient_tensor\(pmg_laplacian op\);", bare)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is an error with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_has_coefficient_tensor(None) == -1
    assert lib.pmg_laplacian_set_coefficient_tensor(None, None, None) == -1
    assert b"pmg_laplacian_set_coefficient_tensor" in lib.pmg_last_error()


def test_python_and_cpp_layers_carry_the_tensor(built):
    import pmg_dolfinx_amd as pm

    for method in ("set_coefficient_tensor", "has_coefficient_tensor"):
        assert callable(getattr(pm.MatFreeLaplacian, method))
    assert list(inspect.signature(pm.MatFreeLaplacian.set_coefficient_tensor).parameters) == ["self", "t"]
    assert list(inspect.signature(pm.MatFreeLaplacian.has_coefficient_tensor).parameters) == ["self"]
    p = inspect.signature(pm.PoissonHierarchy.__init__).parameters
    assert "kappa_tensor" in p and p["kappa_tensor"].default is None
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "void set_coefficient_tensor(std::span<const T> kt)" in hpp
    assert "void clear_coefficient_tensor()" in hpp and "bool has_coefficient_tensor() const" in hpp


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def _reference_gradients(P):
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
    return gr, w3, dN


def _dense_first_principles(mesh, P, kappa, T):
    """(K, M): K[i, j] = sum_cells sum_q w_q |det J_q| kappa_c grad phi_i(x_q) . K_c grad phi_j(x_q), the
    GLL-collocated stiffness matrix written down from the weak form (physical gradients J^-T grad_ref, no adjugate, no
    stored tensor), without boundary conditions; M[i] = sum w_q |det J_q| at the point of dof i, the lumped mass."""
    nd = P + 1
    gr, w3, dN = _reference_gradients(P)
    dofmap = mesh.dofmap(P)
    n = mesh.ndofs(P)
    K, M = np.zeros((n, n)), np.zeros(n)
    Tf = tr.full(T)
    for c in range(mesh.ncells):
        xc = mesh.xgeom[mesh.geom_dofmap[c]]  # [8, 3]
        dofs = dofmap[c]
        for q in range(nd**3):
            J = np.einsum("kd,rk->dr", xc, dN[:, q, :])  # J[d, r] = d x_d / d xi_r
            g = np.linalg.solve(J.T, gr[:, q, :])        # physical gradients [3, i]
            wd = w3[q] * abs(np.linalg.det(J))
            K[np.ix_(dofs, dofs)] += wd * kappa[c] * (g.T @ Tf[c] @ g)
            M[dofs[q]] += wd
    return K, M


def test_with_tensor_is_the_full_tensor_operator():
    """Twisted 2 x 2 x 2 cells at P = 2, a random per-cell kappa and the rotating tensor: the oracle with its tensor
    replaced equals the weak-form matrix to 1e-12 of the largest entry, and is not the scalar operator."""
    P = 2
    mesh = po.BoxMesh((2, 2, 2), warp=twist)
    rng = np.random.default_rng(0)
    kappa = rng.uniform(1.0, 3.0, mesh.ncells)
    T = tr.rotating_tensor(tr.cell_centres(mesh.xgeom, mesh.geom_dofmap))
    nobc = np.zeros(mesh.ndofs(P), dtype=np.int8)
    A = tr.laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc)
    plain = A.assemble_csr().toarray()
    M = tr.with_tensor(A, T).assemble_csr().toarray()
    K, _ = _dense_first_principles(mesh, P, kappa, T)
    scale = np.abs(K).max()
    print(f"with_tensor vs weak form: {np.abs(M - K).max() / scale:.3e}; scalar operator vs weak form: "
          f"{np.abs(plain - K).max() / scale:.3e}")
    assert np.abs(M - K).max() < 1e-12 * scale
    assert np.abs(plain - K).max() > 1e-2 * scale  # the tensor is seen
    # the identity tensor gives the scalar operator back
    eye = np.tile([1.0, 0, 0, 1.0, 0, 1.0], (mesh.ncells, 1))
    assert np.abs(tr.tensor_G(P, mesh.xgeom, mesh.geom_dofmap, eye)
                  - po.Laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc).G).max() < 1e-13
    # symmetric, positive semi-definite with the constants as its only null space
    assert np.abs(M - M.T).max() < 1e-13 * scale
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert abs(ev[0]) < 1e-11 * ev[-1] and ev[1] > 1e-6 * ev[-1]
    # apply and diagonal of the oracle are those of that matrix
    u = rng.standard_normal(mesh.ndofs(P))
    assert np.abs(A.apply(u) - K @ u).max() < 1e-12 * np.abs(K @ u).max()
    assert np.abs(A.diagonal() - np.diag(K)).max() < 1e-12 * np.diag(K).max()
    # the nodal field on top multiplies point by point
    kq = rng.uniform(0.5, 2.0, mesh.ndofs(P))
    G1 = A.G.copy()
    tr.with_tensor(A, T, kq)
    assert np.array_equal(A.G, G1 * kq[A.dofmap][:, :, None])
    # with Dirichlet rows it is symmetric positive definite on the free rows
    bc = mesh.boundary_marker(P)
    B = tr.with_tensor(tr.laplacian(P, kappa, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, bc), T)
    Mb = B.assemble_csr().toarray()
    free = ~bc.astype(bool)
    assert np.abs(Mb[np.ix_(free, free)] - K[np.ix_(free, free)]).max() < 1e-12 * scale
    assert np.array_equal(Mb[~free][:, ~free], np.eye(int((~free).sum())))
    assert np.abs(Mb - Mb.T).max() < 1e-13 * scale and np.linalg.eigvalsh(0.5 * (Mb + Mb.T)).min() > 0


def test_component_order_reproduces_a_quadratic():
    """A sheared box of (2, 3, 2) cells at P = 3 and one constant tensor: for the quadratic
    u = x^2 + 2xy - yz + 3z^2 + x - y the GLL rule integrates every term of the weak form exactly, so the interior
    rows of A u - M f vanish with f = -sum_ij K_ij d_ij u (a constant).  Swapping the xy and xz components breaks it:
    the order (xx, xy, xz, yy, yz, zz) is observable."""
    P = 3
    shear = np.array([[1.0, 0.2, 0.1], [0.0, 0.8, 0.3], [0.1, 0.0, 1.3]])
    mesh = po.BoxMesh((2, 3, 2), warp=lambda x: x @ shear.T)
    Kc = np.array([[2.0, 0.3, -0.5], [0.3, 1.0, 0.7], [-0.5, 0.7, 3.0]])
    assert np.linalg.eigvalsh(Kc).min() > 0
    c = mesh.dof_coordinates(P)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    u = x**2 + 2 * x * y - y * z + 3 * z**2 + x - y
    hess = np.array([[2.0, 2.0, 0.0], [2.0, 0.0, -1.0], [0.0, -1.0, 6.0]])
    f = -np.sum(Kc * hess)
    gr, w3, dN = _reference_gradients(P)
    M = np.zeros(mesh.ndofs(P))
    for cell in range(mesh.ncells):
        xc = mesh.xgeom[mesh.geom_dofmap[cell]]
        for q in range((P + 1) ** 3):
            J = np.einsum("kd,rk->dr", xc, dN[:, q, :])
            M[mesh.dofmap(P)[cell, q]] += w3[q] * abs(np.linalg.det(J))
    nobc = np.zeros(mesh.ndofs(P), dtype=np.int8)
    interior = ~mesh.boundary_marker(P).astype(bool)
    T = np.tile(tr.packed(Kc[None])[0], (mesh.ncells, 1))
    A = tr.with_tensor(tr.laplacian(P, 1.0, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc), T)
    Au = A.apply(u)
    good = np.abs(Au - M * f)[interior].max() / np.abs(Au).max()
    swapped = T[:, [0, 2, 1, 3, 4, 5]]
    Aw = tr.with_tensor(tr.laplacian(P, 1.0, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc), swapped)
    bad = np.abs(Aw.apply(u) - M * f)[interior].max() / np.abs(Au).max()
    print(f"interior rows of A u - M f: {good:.3e}; with xy and xz swapped: {bad:.3e}")
    assert good < 1e-12
    assert bad > 1e-3


def test_tensors_of_the_tests_are_positive_definite():
    c = np.random.default_rng(1).uniform(0, 1, (50, 3))
    R = tr.full(tr.rotating_tensor(c))
    ev = np.linalg.eigvalsh(R)
    assert np.allclose(ev[:, 0], 1.0) and np.allclose(ev[:, 1], 2.0 + c[:, 0]) and np.allclose(ev[:, 2], 4.0)
    S = tr.random_spd(40, 3)
    ev = np.linalg.eigvalsh(tr.full(S))
    assert ev.min() >= 0.5 - 1e-12 and ev.max() <= 2.0 + 1e-12
    assert np.abs(S[:, [1, 2, 4]]).min() > 1e-3
    assert np.array_equal(tr.random_spd(40, 3), S) and not np.array_equal(tr.random_spd(40, 4), S)
