"""--reaction S in the C++ drivers (examples/, over include/pmg_amd.hpp): the reaction term sigma u with
sigma_c = S (1 + x_c) at the cell centre, set through acc::MatFreeLaplacian<T>::set_reaction.  The drivers run as
separate processes that link libpmg_amd.so."""
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


def test_mat_free_driver_against_csr_and_reference(gpu):
    """The matrix-free apply with the term against the driver's own assembled operator, at the bound
    tests/test_gpu_coefficient_tensor_drivers.py applies to that comparison (1e-12 |y|), and |y| against the reference
    with the same coefficient -- which is not the |y| of the operator without the term."""
    from oracle import pmg_oracle as po

    n, P, S = 4, 3, 3.0
    out = run("mat_free_main", "--n", n, "--degree", P, "--mat_comp", "--nreps", 3, "--reaction", S)
    (ny,) = grab(r"Norm of y = (\S+)", out)
    (nz,) = grab(r"Norm of z = (\S+)", out)
    (err,) = grab(r"Norm of error = (\S+)", out)
    print(f"mat_free_main --reaction {S}: |y| {ny:.6e} |z| {nz:.6e} error {err:.3e}")
    assert err < 1e-12 * ny
    mesh = po.BoxMesh(n)
    c = mesh.dof_coordinates(P)
    sigma = rr.linear_sigma(S)(mesh.xgeom[mesh.geom_dofmap].mean(axis=1))
    A = rr.laplacian(P, 2.0, sigma, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P))
    u = np.sin(1.0 + 3 * c[:, 0] + 5 * c[:, 1] * c[:, 2])
    assert abs(ny - np.linalg.norm(A.apply(u))) < 1e-12 * ny
    assert abs(ny - np.linalg.norm(A.A.apply(u))) > 1e-6 * ny


@pytest.mark.parametrize("fp32_cycle", [False, True])
def test_pmg_driver_converges(gpu, fp32_cycle):
    out = run("pmg_main", "--n", 8, "--orders", "1,2,4", "--amg", "--pcg", "--reaction", 3,
              *(["--fp32-cycle"] if fp32_cycle else []))
    assert "AMG coarse solver:" in out
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    print(m.group(0))
    assert int(m.group(1)) < 100 and float(m.group(2)) < 1e-6  # the driver's own limits: 100 iterations, rtol 1e-8
