"""The assembled CSR operator (``pmg_matrix``, ``MatrixOperator``; acc::MatrixOperator of src/csr.hpp) against the
oracle's ``Laplacian.assemble_csr`` and against the library's own matrix-free operator: matrix, product, node order,
kappa, the solvers on it, assembled levels inside the V-cycle, and the refusals.

Tolerances are DESIGN.md section 2's: 1e-12 relative per operator application (and per matrix entry, relative to
max |A|), 1e-10 for iterates after full cycles / solves, 1e-8 for residual norms and eigenvalue estimates."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(6, 1), (4, 2), (3, 3), (3, 4), (2, 5), (2, 6), (2, 7), (2, 8)]


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


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


def _kappa(ncells):
    return 1.0 + 0.5 * np.sin(1.7 * np.arange(ncells) + 0.3)  # varies per cell, in [0.5, 1.5]


class Problem:
    """One level on the warped box: the device operator (per-cell kappa, standard boundary marker) and its oracle."""

    def __init__(self, pm, n, P, node_order="ascending"):
        from oracle import pmg_oracle as po

        self.gm = po.BoxMesh(n, warp=warp)
        self.part = pm.BoxPartition(n, warp=warp)
        self.lv = lv = self.part.level(P)
        assert np.array_equal(lv.dofmap.reshape(-1), self.gm.dofmap(P).reshape(-1))
        self.layout = pm.make_layout(lv)
        self.kappa = _kappa(self.part.ncells)
        dofmap = lv.dofmap
        if node_order == "basix":
            dofmap = pm.dofmap_in_node_order(lv.dofmap, pm.basix_node_permutation(P))
        self.op = pm.MatFreeLaplacian(P, self.kappa, dofmap, self.part.xgeom, self.part.geom_dofmap, lv.lcells,
                                      lv.bcells, lv.bc_marker, self.layout, node_order=node_order)
        self.P = P

    def oracle(self, kappa=None):
        from oracle import pmg_oracle as po

        gm = self.gm
        return po.Laplacian(self.P, self.kappa if kappa is None else kappa, gm.dofmap(self.P), gm.xgeom,
                            gm.geom_dofmap, gm.boundary_marker(self.P))


def _pattern_pairs(dofmap, N):
    dm = np.asarray(dofmap, dtype=np.int64).reshape(-1, N)
    rows = np.repeat(dm, N, axis=1).ravel()
    cols = np.tile(dm, (1, N)).ravel()
    return np.unique(rows * (dm.max() + 1) + cols).size


@pytest.mark.parametrize("n,P", CASES)
def test_matrix_against_oracle(pm, n, P):
    pr = Problem(pm, n, P)
    M = pm.MatrixOperator(pr.op)
    A = pr.oracle()
    ref = A.assemble_csr()
    got = M.to_scipy()
    amax = np.abs(ref.data).max()
    diff = abs(got - ref)
    err = diff.max() if diff.nnz else 0.0
    print(f"n={n} P={P}: rows {M.rows} nnz {M.nnz} max|A| {amax:.3e} max|diff| {err:.3e}")
    assert got.shape == ref.shape == (pr.lv.ndofs, pr.lv.ndofs) and M.rows == pr.lv.ndofs
    assert err <= 1e-12 * amax
    # the pattern: dolfinx's, every pair of dofs that shares a cell; sorted columns, int32
    N = (P + 1) ** 3
    assert M.nnz == _pattern_pairs(pr.lv.dofmap, N)
    rp, ci, v = M.export()
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and rp[0] == 0 and rp[-1] == M.nnz == ci.size == v.size
    d, starts = np.diff(ci), rp[1:-1]
    within = np.ones(d.size, dtype=bool)
    within[starts[(starts > 0) & (starts < ci.size)] - 1] = False  # differences across a row boundary
    assert np.all(d[within] > 0)
    # Dirichlet rows are unit rows (and, by symmetry below, Dirichlet columns are zero elsewhere)
    bc = np.asarray(pr.lv.bc_marker).astype(bool)
    assert bc.any()
    sub = got[np.flatnonzero(bc)]
    assert np.array_equal(got.diagonal()[bc], np.ones(bc.sum()))
    assert abs(sub).sum() == bc.sum()
    sym = abs(got - got.T)
    assert (sym.max() if sym.nnz else 0.0) <= 1e-13 * amax
    # the "A norm" of src/csr.hpp:95-99: Frobenius norm over the same pattern
    fro = np.sqrt((ref.data ** 2).sum())
    assert abs(M.norm() - fro) <= 1e-12 * fro


@pytest.mark.parametrize("n,P", CASES)
def test_product_and_diagonal(pm, n, P):
    pr = Problem(pm, n, P)
    M = pm.MatrixOperator(pr.op)
    A = pr.oracle()
    u = np.random.default_rng(100 + P).standard_normal(pr.lv.ndofs)
    x, y, z = _vec(pm, pr.layout, u), pm.Vector(pr.layout), pm.Vector(pr.layout)
    y.set(-3.0)  # the product overwrites its output
    M(x, y)
    e_oracle = _relerr(y.data_copy(), A.apply(u))
    pr.op(x, z)  # the reference's --mat_comp, examples/mat_free/main.cpp:270-288
    e_free = _relerr(y.data_copy(), z.data_copy())
    pr.op.compute_diag_inverse()
    d0, d1 = pm.Vector(pr.layout), pm.Vector(pr.layout)
    pr.op.get_diag_inverse(d0)
    M.get_diag_inverse(d1)
    e_diag = _relerr(d1.data_copy(), d0.data_copy())
    print(f"n={n} P={P}: product vs oracle {e_oracle:.3e}, vs matrix-free {e_free:.3e}, diag {e_diag:.3e}")
    assert e_oracle < 1e-12 and e_free < 1e-12 and e_diag < 1e-12
    assert _relerr(d1.data_copy(), A.diag_inverse()) < 1e-12


@pytest.mark.parametrize("n,P", [(4, 2), (3, 4)])
def test_node_order_does_not_change_the_matrix(pm, n, P):
    a = pm.MatrixOperator(Problem(pm, n, P).op).to_scipy()
    pb = Problem(pm, n, P, node_order="basix")
    assert pb.op.node_order == 1
    b = pm.MatrixOperator(pb.op).to_scipy()
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    err = np.abs(a.data - b.data).max()
    print(f"P={P}: endpoints-first vs ascending {err:.3e}")
    assert err <= 1e-14 * np.abs(a.data).max()


@pytest.mark.parametrize("n,P", [(6, 1), (3, 3)])
def test_kappa_is_read_at_assembly(pm, n, P):
    pr = Problem(pm, n, P)
    M = pm.MatrixOperator(pr.op)
    first = M.export()[2].copy()
    M.update_values()
    assert np.array_equal(M.export()[2], first)  # row-wise gather: two assemblies give the same bits
    u = np.random.default_rng(7).standard_normal(pr.lv.ndofs)
    x, y = _vec(pm, pr.layout, u), pm.Vector(pr.layout)
    M(x, y)
    before = y.data_copy()
    kappa2 = pr.kappa[::-1].copy() * 1.5
    pr.op.kappa.copy_(torch.from_numpy(kappa2))  # in place: the array the operator was created with
    M(x, y)
    assert np.array_equal(y.data_copy(), before)  # the matrix still holds the old kappa
    z = pm.Vector(pr.layout)
    pr.op(x, z)
    assert _relerr(z.data_copy(), before) > 1e-3  # ... the matrix-free operator reads the new one
    M.update_values()
    ref = pr.oracle(kappa2).assemble_csr()
    diff = abs(M.to_scipy() - ref)
    assert (diff.max() if diff.nnz else 0.0) <= 1e-12 * np.abs(ref.data).max()
    M(x, y)
    assert _relerr(y.data_copy(), z.data_copy()) < 1e-12
    d = pm.Vector(pr.layout)
    M.get_diag_inverse(d)  # refreshed with the values
    assert _relerr(d.data_copy(), pr.oracle(kappa2).diag_inverse()) < 1e-12


@pytest.mark.parametrize("n,P", [(6, 1), (3, 3)])
def test_solvers_on_the_matrix(pm, n, P):
    pr = Problem(pm, n, P)
    pr.op.compute_diag_inverse()
    M = pm.MatrixOperator(pr.op)
    rng = np.random.default_rng(11 + P)
    bc = np.asarray(pr.lv.bc_marker).astype(bool)
    b = rng.standard_normal(pr.lv.ndofs)
    b[bc] = 0.0

    def cg_run(A):
        cg = pm.CGSolver(pr.layout)
        cg.set_max_iterations(15)
        cg.set_tolerance(1e-6)
        cg.store_coefficients(True)
        x = pm.Vector(pr.layout)
        x.set(0.0)
        its = cg.solve(A, x, _vec(pm, pr.layout, b))
        return its, x.data_copy(), cg.alphas().copy(), cg.betas().copy(), np.sort(cg.compute_eigenvalues())

    i0, x0, a0, b0, e0 = cg_run(pr.op)
    i1, x1, a1, b1, e1 = cg_run(M)
    print(f"P={P}: CG {i0} / {i1} iterations, iterate {_relerr(x1, x0):.3e}, alphas {_relerr(a1, a0):.3e}, "
          f"betas {_relerr(b1, b0):.3e}, eigenvalues {_relerr(e1, e0):.3e}")
    assert i0 == i1 and a0.size == a1.size
    assert _relerr(x1, x0) < 1e-10
    assert np.all(np.abs(a1 - a0) <= 1e-9 * np.abs(a0)) and np.all(np.abs(b1 - b0) <= 1e-9 * np.abs(b0))
    assert np.all(np.abs(e1 - e0) <= 1e-8 * np.abs(e0))

    def cheb_run(A):
        sm = pm.Chebyshev(pr.layout, (0.1 * e0[-1], 1.1 * e0[-1]))
        sm.set_max_iterations(4)
        x = _vec(pm, pr.layout, np.where(bc, 0.0, 0.05))
        sm.solve(A, x, _vec(pm, pr.layout, b))
        return x.data_copy()

    c0, c1 = cheb_run(pr.op), cheb_run(M)
    print(f"P={P}: Chebyshev iterate {_relerr(c1, c0):.3e}")
    assert _relerr(c1, c0) < 1e-10


# ---- assembled levels in the V-cycle ----
N_H, ORDERS, K = 6, (1, 2, 4), 3
LEVEL_SETS = [(0,), (0, 1), (0, 1, 2)]


def _oracle_cycles(h, cycles):
    from oracle import pmg_oracle as po

    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(N_H, ORDERS, cheb_its=K, warp=warp)
    for s, e in zip(sm, h.eig_ranges):  # same smoother bounds: only the cycle arithmetic is compared
        s.eig_range = e
    x, rn = np.zeros_like(b), []
    for _ in range(cycles):
        x = mg.apply(b, x, compute_rnorm=True)
        rn.append(mg.rnorm)
    return x, rn


@pytest.mark.parametrize("levels", LEVEL_SETS)
def test_cycle_with_assembled_levels(pm, levels):
    h = pm.PoissonHierarchy(N_H, ORDERS, kappa=2.0, cheb_its=K, warp=warp, assembled_levels=levels)
    assert sorted(h.matrices) == list(levels)
    h.mg.set_graph(False)
    x = h.new_vector()
    x.set(0.0)
    rn = [h.mg.apply(h.rhs[-1], x, verbose=True) for _ in range(3)]
    ref, rn_ref = _oracle_cycles(h, 3)
    print(f"levels {levels}: iterate {_relerr(x.data_copy(), ref):.3e}, residual norms {rn} / {rn_ref}")
    assert _relerr(x.data_copy(), ref) < 1e-10
    for a, b in zip(rn, rn_ref):
        assert abs(a - b) < 1e-8 * b

    # stiffness launches and application counts of one cycle, against the all-matrix-free hierarchy
    plain = pm.PoissonHierarchy(N_H, ORDERS, kappa=2.0, cheb_its=K, warp=warp)
    plain.mg.set_graph(False)

    def profile(H):
        for op in H.operators:
            op.set_profiling(True)
            op.read_profile()
        y = H.new_vector()
        y.set(0.0)
        H.mg.apply(H.rhs[-1], y)
        torch.cuda.synchronize()
        launches = [op.read_profile()[1] for op in H.operators]
        for op in H.operators:
            op.set_profiling(False)
        return launches, H.mg.apply_counts()

    l_mixed, c_mixed = profile(h)
    l_plain, c_plain = profile(plain)
    print(f"levels {levels}: stiffness launches {l_mixed} (matrix-free {l_plain}), apply counts {c_mixed}")
    assert c_mixed == c_plain and all(c > 0 for c in c_plain)
    for i in range(len(ORDERS)):
        assert l_mixed[i] == (0 if i in levels else l_plain[i]) and l_plain[i] > 0


def test_graph_key_holds_the_level_matrices(pm):
    """A cycle replayed before ``set_level_matrix``, one after it and one after ``set_level_matrix(level, None)`` each
    match the eager cycle of the same configuration.

    Bound: 1e-12, the project's graph-against-eager bound (tests/test_gpu_distributed.py).  Bit equality cannot be
    asked: the merged launch of a small matrix-free level accumulates with atomics, so two eager cycles already differ
    in the last bits (printed below).  To let that bound tell a stale graph from a fresh one, the level matrix is
    assembled with 1.5 kappa (its smoother then applies 2/3 of the coarse correction): the two configurations differ by
    orders of magnitude more than the bound, which is asserted first."""
    h = pm.PoissonHierarchy(N_H, ORDERS, kappa=2.0, cheb_its=K, warp=warp)
    M = pm.MatrixOperator(h.operators[0])
    h.kappa.mul_(1.5)
    M.update_values()
    h.kappa.div_(1.5)  # 2.0 * 1.5 / 1.5 == 2.0 exactly: the matrix-free operators are what they were
    x = h.new_vector()

    def two_cycles():
        x.set(0.0)
        h.mg.apply(h.rhs[-1], x)
        h.mg.apply(h.rhs[-1], x)
        torch.cuda.synchronize()
        return x.data_copy()

    h.mg.set_graph(False)
    eager_free = two_cycles()
    eager_again = two_cycles()
    h.mg.set_level_matrix(0, M)
    eager_mat = two_cycles()
    h.mg.set_level_matrix(0, None)
    apart = _relerr(eager_mat, eager_free)
    print(f"eager vs eager {_relerr(eager_again, eager_free):.3e}; matrix vs matrix-free configuration {apart:.3e}")
    assert _relerr(eager_again, eager_free) < 1e-12
    assert apart > 1e-6  # a stale graph would be off by this much
    # replay forced on; the same (rhs, y) pair throughout, so only the key separates the graphs
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    g_free = two_cycles()
    h.mg.set_level_matrix(0, M)
    g_mat = two_cycles()
    h.mg.set_level_matrix(0, None)
    g_free2 = two_cycles()
    assert h.mg.graph_replays() - n0 >= 6
    h.mg.set_graph(False)
    print(f"graph vs eager: {_relerr(g_free, eager_free):.3e} {_relerr(g_mat, eager_mat):.3e} "
          f"{_relerr(g_free2, eager_free):.3e}")
    assert _relerr(g_free, eager_free) < 1e-12
    assert _relerr(g_mat, eager_mat) < 1e-12
    assert _relerr(g_free2, eager_free) < 1e-12


def test_pcg_with_a_mixed_hierarchy(pm):
    def run(levels):
        h = pm.PoissonHierarchy(N_H, ORDERS, kappa=2.0, cheb_its=K, warp=warp, assembled_levels=levels)
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(50)
        cg.set_tolerance(1e-8)
        x = h.new_vector()
        x.set(0.0)
        its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
        r = h.new_vector()
        h.operators[-1](x, r)
        b = h.rhs[-1].data_copy()
        return its, x.data_copy(), np.linalg.norm(b - r.data_copy()) / np.linalg.norm(b)

    i0, x0, r0 = run(())
    i1, x1, r1 = run((0, 1))
    print(f"PCG: {i0} / {i1} iterations, residuals {r0:.3e} / {r1:.3e}, iterate {_relerr(x1, x0):.3e}")
    assert i0 == i1 and 1 <= i1 < 50
    assert r0 < 1e-6 and r1 < 1e-6  # true residual after stopping on r.M^-1 r at 1e-8: the bound of test_pmg_driver


# ---- refusals: PMG_ERR_INVALID, a message, no handle ----
def _refused_create(pm, op):
    from pmg_dolfinx_amd import _lib

    h = _lib.vp()
    rc = _lib.lib().pmg_matrix_create_from_laplacian(C.byref(h), op.handle, _lib.current_stream())
    msg = _lib.lib().pmg_last_error().decode()
    return rc, msg, h.value


def test_refused_layout_with_ghosts(pm):
    part = pm.BoxPartition(4, (2, 1, 1), 0, warp=warp)  # rank 0 of two, built in-process
    lv = part.level(2)
    assert lv.num_ghosts > 0
    layout = pm.make_layout(lv)
    op = pm.MatFreeLaplacian(2, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    rc, msg, handle = _refused_create(pm, op)
    assert rc == -1 and handle is None and "single-domain" in msg and "follow-up" in msg
    with pytest.raises(pm._lib.PmgError, match="single-domain"):
        pm.MatrixOperator(op)


def test_refused_batched_geometry(pm):
    from pmg_dolfinx_amd import _lib

    pr = Problem(pm, 4, 2)
    M = pm.MatrixOperator(pr.op)
    _lib.call("pmg_laplacian_set_geometry_batch", pr.op.handle, 8)
    rc, msg, handle = _refused_create(pm, pr.op)
    assert rc == -1 and handle is None and "batched" in msg
    with pytest.raises(_lib.PmgError, match="batched"):
        M.update_values()  # the tensor it would read is gone
    _lib.call("pmg_laplacian_set_geometry_batch", pr.op.handle, 0)
    M.update_values()


def test_refused_fp32_with_a_level_matrix(pm):
    from pmg_dolfinx_amd import _lib

    h = pm.PoissonHierarchy(4, (1, 2), kappa=2.0, cheb_its=2, warp=warp)
    M = pm.MatrixOperator(h.operators[0])
    h.mg.set_level_matrix(0, M)
    with pytest.raises(_lib.PmgError, match="FP32") as e:
        h.mg.set_precision("fp32")
    assert "code -1" in str(e.value) and h.mg.precision == "fp64"
    h.mg.set_level_matrix(0, None)
    h.mg.set_precision("fp32")
    with pytest.raises(_lib.PmgError, match="FP32") as e:
        h.mg.set_level_matrix(0, M)
    assert "code -1" in str(e.value)
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(h.rhs[-1], x)  # the FP32 cycle still runs, matrix-free
    h.mg.set_precision("fp64")
    h.mg.set_level_matrix(0, M)
    with pytest.raises(_lib.PmgError, match="layout"):
        h.mg.set_level_matrix(1, M)


# ---- the C++ drivers over the adapter header (acc::MatrixOperator<T>) ----
def _run(exe, *args):
    import os
    import subprocess

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pmg-dolfinx_amd", "bin", exe)
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _grab(pattern, text):
    import re

    return [float(v) for v in re.findall(pattern, text)]


def test_mat_free_driver_compares_with_the_assembled_operator(pm):
    out = _run("mat_free_main", "--n", 4, "--degree", 3, "--mat_comp", "--nreps", 3)
    (ny,) = _grab(r"Norm of y = (\S+)", out)
    (nz,) = _grab(r"Norm of z = (\S+)", out)
    (err,) = _grab(r"Norm of error = (\S+)", out)
    (nnz,) = _grab(r"CSR nnz = (\d+)", out)
    assert len(_grab(r"CSR Matvec: \d+ reps, (\S+) us per apply", out)) == 1
    print(f"mat_free_main P=3: |y| {ny:.6e} |z| {nz:.6e} error {err:.3e} nnz {int(nnz)}")
    assert err < 1e-12 * ny and nnz == _box_nnz(4, 3)
    out1 = _run("mat_free_main", "--n", 8, "--degree", 1, "--mat_comp", "--nreps", 3)
    assert len(_grab(r"Norm of error = (\S+)", out1)) == 1  # the stencil comparison keeps its lines
    (e1,) = _grab(r"CSR error norm = (\S+)", out1)
    (y1,) = _grab(r"Norm of y = (\S+)", out1)
    assert e1 < 1e-12 * y1


def _box_nnz(n, P):
    """nnz of the pattern on an n^3 box: per direction, a vertex dof couples to 2P+1 (P+1 at the ends) and an
    interior dof to P+1 dofs; the 3-D pattern is the tensor product."""
    one = (n - 1) * (2 * P + 1) + 2 * (P + 1) + n * (P - 1) * (P + 1)
    return one ** 3


def test_pmg_driver_on_assembled_levels(pm):
    from oracle import pmg_oracle as po

    n, orders, k, cycles = 6, (1, 2, 4), 3, 4
    out = _run("pmg_main", "--n", n, "--orders", ",".join(map(str, orders)), "--smoother-its", k, "--cycles", cycles,
               "--csr")
    lam = _grab(r"Eigenvalues level \d+: \S+ - (\S+)", out)
    rn = _grab(r"Cycle \d+: residual norm = (\S+)", out)
    nnz = _grab(r"Level \d+: CSR nnz = (\d+)", out)
    assert len(lam) == len(orders) and len(rn) == cycles
    assert nnz == [_box_nnz(n, P) for P in orders]
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=k)
    for got, ref in zip(lam, eigs):
        assert abs(1.1 * got - ref[1]) < 1e-8 * ref[1]
    for s, l in zip(sm, lam):
        s.eig_range = (0.1 * l, 1.1 * l)
    x = np.zeros_like(b)
    for c in range(cycles):
        x = mg.apply(b, x, compute_rnorm=True)
        assert abs(rn[c] - mg.rnorm) < 1e-8 * mg.rnorm + 1e-13, (c, rn[c], mg.rnorm)
    # a list of levels: only those are assembled
    some = _run("pmg_main", "--n", n, "--orders", "1,2,4", "--smoother-its", k, "--cycles", 1, "--csr", "0,2")
    assert [int(v) for v in _grab(r"Level (\d+): CSR nnz", some)] == [0, 2]


def test_cg_driver_eigenvalue_estimate_on_the_assembled_operator(pm):
    args = ("--n", 6, "--degree", 3)
    out = _run("cg_main", *args, "--csr")
    assert "CSR nnz = " in out
    a = _grab(r"Using eig range:\S+ - (\S+)", _run("cg_main", *args))
    b = _grab(r"Using eig range:\S+ - (\S+)", out)
    print(f"cg_main eig range upper bound: {a} / {b}")
    assert len(a) == len(b) == 1 and abs(a[0] - b[0]) < 1e-8 * a[0]
