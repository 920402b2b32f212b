"""The C++ drivers with --csr on several ranks: examples/pmg/run_ranks.sh starts pmg_main / cg_main as two processes
on the one GPU of the box (--comm windows), where acc::MatrixOperator<T> takes the distributed constructor.  The same
global problem as the single-process run, so the same numbers; bounds as in tests/test_gpu_drivers.py
(test_pmg_driver_ranks_share_the_gpu_through_the_window_communicator,
test_cg_and_vector_update_drivers_as_ranks_sharing_the_gpu)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pmg-dolfinx_amd", "bin")
SCRIPT = os.path.join(ROOT, "examples", "pmg", "run_ranks.sh")
PMG_ARGS = ["--n", "8", "--orders", "1,2,4", "--smoother-its", "3", "--cycles", "4"]


def run(exe, *args):
    path = os.path.join(BIN, exe)
    assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def ranks(exe, *args):
    r = subprocess.run(["bash", SCRIPT, "1,1,2", *map(str, args), "--comm", "windows"], capture_output=True, text=True,
                       timeout=300,
                       env={**os.environ, "PMG_MAIN": os.path.join(BIN, exe), "PMG_WINDOW_TIMEOUT_MS": "20000"})
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def grab(pattern, text):
    return [float(v) for v in re.findall(pattern, text)]


def test_pmg_driver_with_every_level_assembled_as_two_ranks(built):
    """The same arithmetic as the single process: the residuals cycle by cycle to 1e-9 of the first; the A norm the
    root prints is the global one."""
    one, two = run("pmg_main", *PMG_ARGS, "--csr"), ranks("pmg_main", *PMG_ARGS, "--csr")
    r1, r2 = (grab(r"Cycle \d+: residual norm = (\S+)", out) for out in (one, two))
    assert len(r1) == len(r2) == 4
    assert all(abs(a - b) < 1e-9 * r1[0] for a, b in zip(r1, r2)), (r1, r2)
    n1, n2 = (grab(r"Level \d+: CSR nnz = \d+, A norm = (\S+)", out) for out in (one, two))
    assert len(n1) == len(n2) == 3
    assert all(abs(a - b) < 1e-12 * a for a, b in zip(n1, n2)), (n1, n2)


def test_pmg_driver_assembled_coarse_level_replayed_under_pcg(built):
    out = ranks("pmg_main", *PMG_ARGS, "--csr", "0", "--graph", "--pcg")
    assert "(hipGraph replays)" in out
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    assert m and float(m.group(2)) < 1e-6


def test_cg_driver_on_the_assembled_operator_as_two_ranks(built):
    one, two = run("cg_main", "--n", 6, "--degree", 3, "--csr"), ranks("cg_main", "--n", 6, "--degree", 3, "--csr")
    assert grab(r"Number of iterations (\d+)", one) == grab(r"Number of iterations (\d+)", two)
    e1 = re.findall(r"Computed eigs = \(([0-9.e+-]+), ([0-9.e+-]+)\)", one)[0]
    e2 = re.findall(r"Computed eigs = \(([0-9.e+-]+), ([0-9.e+-]+)\)", two)[0]
    assert all(abs(float(a) - float(b)) < 1e-9 * float(e1[1]) for a, b in zip(e1, e2))
    (b1,), (b2,) = grab(r"Norm of b = (\S+)", one), grab(r"Norm of b = (\S+)", two)
    assert abs(b1 - b2) < 1e-11 * b1
