"""--robin A in the C++ drivers (examples/, over include/pmg_amd.hpp): the Dirichlet marker is kept on the face x = 0
only and the other five faces carry a Robin term with alpha = A (1 + y) at their facet points, on every level, set
through acc::MatFreeLaplacian<T>::set_robin.  The drivers run as separate processes that link libpmg_amd.so."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402
import robin_reference as rb  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "pmg-dolfinx_amd", "bin")


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run(exe, *args):
    path = os.path.join(BIN, exe)
    assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def grab(pattern, text):
    return [float(v) for v in re.findall(pattern, text)]


def _level_operator(part, P, A, kappa=2.0, S=0.0):
    """The driver's operator of degree P: marker on x = 0, alpha = A (1 + y) on the other five faces, and
    sigma_c = S (1 + x_c) if S > 0."""
    lv = part.level(P)
    bc = rb.one_face_marker(lv.bc_marker, part.dof_coordinates(P))
    cells, facets = part.exterior_facets()
    keep = facets != 0
    cells, facets = cells[keep], facets[keep]
    alpha = rb.linear_alpha(A)(part.facet_point_coordinates(P, cells, facets).reshape(-1, 3)).reshape(cells.size, -1)
    sigma = rr.linear_sigma(S)(part.xgeom[part.geom_dofmap].mean(axis=1)) if S > 0 else None
    return rb.laplacian(part, P, kappa, lv.dofmap, bc, cells, facets, alpha, sigma)


def test_mat_free_driver_against_csr_and_reference(gpu):
    """The matrix-free apply with the term against the driver's own assembled operator, at the bound
    tests/test_gpu_reaction_drivers.py applies to that comparison (1e-12 |y|), and |y| against the reference with the
    same marker and coefficient -- which is not the |y| of the operator without the term."""
    import pmg_dolfinx_amd as pm

    n, P, A = 4, 3, 2.0
    out = run("mat_free_main", "--n", n, "--degree", P, "--mat_comp", "--nreps", 3, "--robin", A)
    (ny,) = grab(r"Norm of y = (\S+)", out)
    (nz,) = grab(r"Norm of z = (\S+)", out)
    (err,) = grab(r"Norm of error = (\S+)", out)
    print(f"mat_free_main --robin {A}: |y| {ny:.6e} |z| {nz:.6e} error {err:.3e}")
    assert err < 1e-12 * ny
    part = pm.BoxPartition(n)
    op = _level_operator(part, P, A)
    c = part.dof_coordinates(P)
    u = np.sin(1.0 + 3 * c[:, 0] + 5 * c[:, 1] * c[:, 2])
    assert abs(ny - np.linalg.norm(op.apply(u))) < 1e-12 * ny
    assert abs(ny - np.linalg.norm(op.A.apply(u))) > 1e-6 * ny


@pytest.fixture(scope="module")
def oracle_pcg():
    """Iterations of the oracle's flexible PCG to 1e-8 (the driver's limits) on the driver's problem: the V-cycle
    1 -> 2 -> 4 with three Chebyshev steps and the oracle's own eigenvalue bounds, the coarsest level solved exactly
    (the driver's AMG-preconditioned CG solves it to 1e-5)."""
    cache = {}

    def get(S):
        if S in cache:
            return cache[S]
        import scipy.sparse.linalg as spl

        import pmg_dolfinx_amd as pm
        from oracle import pmg_oracle as po

        n, orders, A = 8, (1, 2, 4), 2.0
        part = pm.BoxPartition(n)
        ops = [_level_operator(part, P, A, S=S) for P in orders]
        sm = [po.Chebyshev(po.estimate_eig_range(op, op.ndofs)[0], 3) for op in ops]
        it = [po.Interpolator(orders[i], orders[i + 1], ops[i].dofmap, ops[i + 1].dofmap, ops[i].ndofs,
                              ops[i + 1].ndofs) for i in range(len(orders) - 1)]
        lu = spl.splu(ops[0].assemble_csr().tocsc())

        def coarse(u0, b0):
            u0[:] = lu.solve(b0)

        mg = po.MultigridPreconditioner(ops, sm, it, ops[0].bc, coarse_solver=coarse)
        b = ops[-1].A.rhs_manufactured(part.dof_coordinates(orders[-1]))
        cg = po.CGSolver()
        cg.set_max_iterations(100)
        cg.set_tolerance(1e-8)
        x = np.zeros_like(b)
        its = cg.solve(ops[-1], x, b, precond=lambda r: mg.apply(r, np.zeros_like(r)), flexible=True)
        res = np.linalg.norm(b - ops[-1].apply(x)) / np.linalg.norm(b)
        cache[S] = (its, res)
        return cache[S]

    return get


@pytest.mark.parametrize("extra,S", [((), 0.0), (("--reaction", 3, "--fp32-cycle"), 3.0)], ids=["robin", "robin-reaction-fp32"])
def test_pmg_driver_converges_with_the_oracles_iteration_count(gpu, oracle_pcg, extra, S):
    out = run("pmg_main", "--n", 8, "--orders", "1,2,4", "--amg", "--pcg", "--robin", 2, *extra)
    assert "AMG coarse solver:" in out
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    its, res = oracle_pcg(S)
    print(m.group(0), f"-- oracle: {its} iterations, residual {res:.3e}")
    assert int(m.group(1)) < 100 and float(m.group(2)) < 1e-6  # the driver's own limits: 100 iterations, rtol 1e-8
    assert int(m.group(1)) == its
