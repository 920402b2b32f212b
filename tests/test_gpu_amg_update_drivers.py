"""--amg-renew in the C++ driver (examples/pmg, over include/pmg_amd.hpp): the AMG is created on the degree-1 operator
before the coefficient options reach it and renewed in place after them (AmgSolver::update_values).  The driver runs
as a separate process that links libpmg_amd.so."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def iterations(out):
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    assert m, out
    assert float(m.group(2)) < 1e-6
    return int(m.group(1))


def test_renewed_hierarchy_serves_the_solve_like_a_fresh_one(gpu):
    args = ("--n", 16, "--orders", "1,2,4", "--amg", "--pcg", "--kappa-tensor")
    fresh, renewed = run("pmg_main", *args), run("pmg_main", *args, "--amg-renew")
    m = re.search(r"AMG renewed in place: (\d+) levels, (\d+) rows, ([0-9.]+) ms", renewed)
    assert m, renewed
    print(m.group(0))
    assert int(m.group(1)) >= 2 and int(m.group(2)) == 17 ** 3
    assert "AMG renewed in place" not in fresh and "AMG coarse solver:" in renewed
    its_fresh, its_renewed = iterations(fresh), iterations(renewed)
    print(f"PCG iterations: fresh hierarchy {its_fresh}, renewed {its_renewed}")
    assert abs(its_fresh - its_renewed) <= 1
