"""The reaction term without a GPU: the two entry points are declared, exported and bound, the Python and C++ layers
carry them, and the CPU truth every GPU test of tests/test_gpu_reaction.py compares against
(tests/reaction_reference.py: the oracle's operator plus one vector d) is the mass matrix of sigma u written down from
the weak form with the GLL rule -- diagonal, with exactly d on it -- and solves a manufactured problem."""
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

import reaction_reference as rr  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

NAMES = ("pmg_laplacian_set_reaction", "pmg_laplacian_has_reaction")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", bare))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_laplacian_set_reaction\(pmg_laplacian op, const double\* sigma, pmg_stream stream\);",
                     bare)
    assert re.search(r"int\s+pmg_laplacian_has_reaction\(pmg_laplacian op\);", bare)
    # the header says what does not change
    assert re.search(r"couples no unmarked row\s+\*?\s*to a marked column", src)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is an error with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_laplacian_has_reaction(None) == -1
    assert lib.pmg_laplacian_set_reaction(None, None, None) == -1
    assert b"pmg_laplacian_set_reaction" in lib.pmg_last_error()


def test_python_and_cpp_layers_carry_the_term(built):
    import pmg_dolfinx_amd as pm

    for method in ("set_reaction", "has_reaction"):
        assert callable(getattr(pm.MatFreeLaplacian, method))
    assert list(inspect.signature(pm.MatFreeLaplacian.set_reaction).parameters) == ["self", "sigma"]
    assert list(inspect.signature(pm.MatFreeLaplacian.has_reaction).parameters) == ["self"]
    p = inspect.signature(pm.PoissonHierarchy.__init__).parameters
    assert "reaction" in p and p["reaction"].default is None
    problem = open(os.path.join(ROOT, "pmg-dolfinx_amd", "problem.py")).read()
    assert problem.index("op.set_reaction(") < problem.index("op.compute_diag_inverse()")
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "void set_reaction(std::span<const T> sigma)" in hpp
    assert "void clear_reaction()" in hpp and "bool has_reaction() const" in hpp
    for driver in ("pmg", "mat_free"):
        src = open(os.path.join(ROOT, "examples", driver, driver + "_main.cpp")).read()
        assert '"--reaction"' in src and "set_reaction(" in src


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def _basis_at_points(P):
    """phi[q, i]: the nd^3 tensor-product Lagrange functions on the GLL nodes, evaluated (not assumed) at the nd^3
    GLL points; the 3-D weights; the trilinear map's vertex gradients dN[3, q, 8]."""
    nd = P + 1
    xi, w = po.gll_points_weights(nd)
    L = po.lagrange_eval_matrix(xi, xi)  # [point, basis]
    phi = np.einsum("ai,bj,ck->abcijk", L, L, L).reshape(nd**3, nd**3)
    w3 = np.einsum("a,b,c->abc", w, w, w).ravel()
    ph, dph = np.stack([1.0 - xi, xi], axis=1), np.stack([-np.ones(nd), np.ones(nd)], axis=1)
    dN = np.stack([np.einsum("ai,bj,cl->abcijl", dph, ph, ph), np.einsum("ai,bj,cl->abcijl", ph, dph, ph),
                   np.einsum("ai,bj,cl->abcijl", ph, ph, dph)]).reshape(3, nd**3, 8)  # vertex k = i*4 + j*2 + l
    return phi, w3, dN


def _dense_mass(mesh, P, sigma):
    """M[i, j] = sum_c sigma_c sum_q w_q |det J_q| phi_i(x_q) phi_j(x_q), no boundary conditions."""
    phi, w3, dN = _basis_at_points(P)
    dofmap = mesh.dofmap(P)
    n = mesh.ndofs(P)
    M = np.zeros((n, n))
    for c in range(mesh.ncells):
        xc = mesh.xgeom[mesh.geom_dofmap[c]]  # [8, 3]
        dofs = dofmap[c]
        for q in range((P + 1) ** 3):
            J = np.einsum("kd,rk->dr", xc, dN[:, q, :])
            M[np.ix_(dofs, dofs)] += sigma[c] * w3[q] * abs(np.linalg.det(J)) * np.outer(phi[q], phi[q])
    return M


def test_reaction_vector_is_the_collocated_mass_matrix():
    """Twisted 2 x 2 x 2 cells at P = 2 and 3: the weak-form mass matrix of sigma u under the GLL rule equals diag(d)
    to 1e-14 of the largest entry, off-diagonals included."""
    mesh = po.BoxMesh((2, 2, 2), warp=twist)
    for P in (2, 3):
        sigma = rr.random_sigma(mesh.ncells, 10 + P)
        assert (sigma == 0).any() and (sigma > 0).sum() >= 4
        nobc = np.zeros(mesh.ndofs(P), dtype=np.int8)
        d = rr.reaction_vector(P, sigma, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc)
        M = _dense_mass(mesh, P, sigma)
        err = np.abs(M - np.diag(d)).max() / np.abs(M).max()
        print(f"P = {P}: weak-form mass matrix vs diag(d): {err:.3e}")
        assert err < 1e-14
        assert d.min() >= 0 and d.max() > 0
        # marked dofs carry none, and the operator's rows there stay y = x
        bc = mesh.boundary_marker(P)
        A = rr.laplacian(P, 0.1, sigma, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, bc)
        marked = bc.astype(bool)
        assert np.array_equal(A.d[marked], np.zeros(int(marked.sum()))) and np.array_equal(A.d[~marked], d[~marked])
        u = np.random.default_rng(P).standard_normal(mesh.ndofs(P))
        y = A.apply(u)
        assert np.array_equal(y[marked], u[marked])
        assert np.abs(y - A.dense() @ u).max() < 1e-12 * np.abs(y).max()
        assert np.abs(A.diagonal() - np.diag(A.dense())).max() < 1e-12 * A.diagonal().max()
        # the term is seen where it lives, on the unmarked rows (kappa = 0.1 and sigma <= 4 on cells of size 1/2)
        assert np.abs(y - A.A.apply(u))[~marked].max() > 1e-2 * np.abs(y[~marked]).max()


def test_reaction_vector_sums_to_sigma_times_volume():
    """An unwarped box with constant sigma and no marked dof: sum(d) = sigma * volume to 1e-13 relative."""
    lo, hi, sigma = (0.0, -1.0, 0.5), (2.0, 0.5, 1.25), 3.7
    volume = float(np.prod(np.subtract(hi, lo)))
    mesh = po.BoxMesh((3, 2, 4), lo=lo, hi=hi)
    for P in (1, 2, 5):
        nobc = np.zeros(mesh.ndofs(P), dtype=np.int8)
        d = rr.reaction_vector(P, np.full(mesh.ncells, sigma), mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc)
        assert abs(d.sum() - sigma * volume) < 1e-13 * sigma * volume


def _manufactured_errors(P, sigma=5.0, n=2):
    """Nodal max errors of the dense solves of (A + D) u_h = b and of A u_h = b, b the GLL load of
    (3 pi^2 + sigma) u, u = sin(pi x) sin(pi y) sin(pi z) on the unit cube, homogeneous Dirichlet."""
    mesh = po.BoxMesh((n, n, n))
    bc = mesh.boundary_marker(P)
    A = rr.laplacian(P, 1.0, np.full(mesh.ncells, sigma), mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, bc)
    c = mesh.dof_coordinates(P)
    u = np.sin(np.pi * c[:, 0]) * np.sin(np.pi * c[:, 1]) * np.sin(np.pi * c[:, 2])
    nobc = np.zeros_like(bc)
    lumped = rr.reaction_vector(P, np.ones(mesh.ncells), mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, nobc)
    b = lumped * (3 * np.pi**2 + sigma) * u
    b[bc.astype(bool)] = 0.0
    with_term = np.linalg.solve(A.dense(), b)
    without = np.linalg.solve(A.A.assemble_csr().toarray(), b)
    return np.abs(with_term - u).max(), np.abs(without - u).max()


def test_manufactured_solution_converges_and_needs_the_term():
    e2, e2_without = _manufactured_errors(2)
    e4, e4_without = _manufactured_errors(4)
    print(f"nodal max error, n = 2: P = 2 {e2:.3e} (without D {e2_without:.3e}), P = 4 {e4:.3e} "
          f"(without D {e4_without:.3e})")
    assert e4 < e2
    assert e2 < e2_without and e4 < e4_without
