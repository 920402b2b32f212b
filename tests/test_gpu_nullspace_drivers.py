"""--neumann in the C++ drivers (examples/, over include/pmg_amd.hpp): no Dirichlet marker on any level, the load made
compatible with acc::remove_mean, the constant null space set on the outer CG, the coarse CG and the AMG.  The drivers
run as separate processes that link libpmg_amd.so.

The manufactured problem of pmg_main (u = cos pi x cos pi y cos pi z on the unit box) is bounded by the same error of
the CPU restatement on that mesh, times 2 (the driver's FP64 rounding against a different iteration count):
RESTATED_ERROR is what

    python tools/nullspace_manufactured.py --n 8 --degree 4

prints (oracle operator, projected Jacobi-CG of tests/nullspace_reference.py at rtol 1e-8; the same to all digits at
rtol 1e-12: it is the discretisation error)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "pmg-dolfinx_amd", "bin")

RESTATED_ERROR = 1.596695e-08


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run(exe, *args, expect=0):
    path = os.path.join(BIN, exe)
    assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == (expect == 0), r.stdout + r.stderr
    return r.stdout + r.stderr


def grab(pattern, text):
    return [float(v) for v in re.findall(pattern, text)]


@pytest.mark.parametrize("extra", [(), ("--amg-cycles", 2, "--graph")], ids=["amg-krylov", "amg-2-cycles-graph"])
def test_pmg_driver_solves_the_manufactured_neumann_problem(gpu, extra):
    out = run("pmg_main", "--n", 8, "--orders", "1,2,4", "--amg", "--pcg", "--neumann", *extra)
    assert "AMG coarse solver:" in out
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    (err,) = grab(r"Neumann manufactured solution: max nodal error = (\S+)", out)
    print(m.group(0), f"-- max nodal error {err:.6e}, restated {RESTATED_ERROR:.6e}, bound {2 * RESTATED_ERROR:.6e}")
    assert int(m.group(1)) < 100 and float(m.group(2)) < 1e-6  # the driver's own limits: 100 iterations, rtol 1e-8
    assert err < 2 * RESTATED_ERROR


def test_pmg_driver_refuses_neumann_with_a_reaction_term(gpu):
    out = run("pmg_main", "--n", 4, "--orders", "1,2", "--neumann", "--reaction", 3, expect=1)
    assert "--neumann with --reaction or --robin" in out and "not singular" in out


def test_mat_free_driver_against_csr_on_the_unmarked_operator(gpu):
    """Matrix-free against the driver's own assembled operator at the bound tests/test_gpu_robin_drivers.py applies to
    that comparison (1e-12 |y|); the vector is not the null vector."""
    out = run("mat_free_main", "--n", 4, "--degree", 3, "--mat_comp", "--nreps", 3, "--neumann")
    (ny,) = grab(r"Norm of y = (\S+)", out)
    (err,) = grab(r"Norm of error = (\S+)", out)
    print(f"mat_free_main --neumann: |y| {ny:.6e} error {err:.3e}")
    assert ny > 0 and err < 1e-12 * ny


def test_cg_driver_converges(gpu):
    out = run("cg_main", "--n", 8, "--neumann")
    m = re.search(r"Neumann CG: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+) \((\w+)", out)
    print(m.group(0))
    assert m.group(3) == "converged" and int(m.group(1)) < 1000
    assert float(m.group(2)) < 1e-4  # rtol 1e-6 on sqrt(r . D^-1 r): the plain residual within the diagonal's spread
