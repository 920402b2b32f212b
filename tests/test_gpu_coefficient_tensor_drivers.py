"""--kappa-tensor in the C++ drivers (examples/, over include/pmg_amd.hpp): the per-cell diffusion tensor with
eigenvalues (1, 2 + x, 4) rotated by Rz(0.6 + 0.8 y) Rx(0.4 + 0.5 z) at the cell centre, set through
acc::MatFreeLaplacian<T>::set_coefficient_tensor.  The drivers run as separate processes that link libpmg_amd.so."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tensor_coefficient_reference as tr  # noqa: E402

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


@pytest.mark.parametrize("with_field", [False, True])
def test_mat_free_driver_against_csr_and_oracle(gpu, with_field):
    """The matrix-free apply with the tensor (and the nodal field on top) against the driver's own assembled
    operator, at the bound tests/test_gpu_matrix_operator.py applies to that comparison (1e-12 |y|), and |y| against
    the oracle with the same coefficient."""
    from oracle import pmg_oracle as po

    n, P = 8, 3
    out = run("mat_free_main", "--n", n, "--degree", P, "--mat_comp", "--nreps", 3, "--kappa-tensor",
              *(["--kappa-field"] if with_field else []))
    (ny,) = grab(r"Norm of y = (\S+)", out)
    (nz,) = grab(r"Norm of z = (\S+)", out)
    (err,) = grab(r"Norm of error = (\S+)", out)
    print(f"mat_free_main --kappa-tensor{' --kappa-field' if with_field else ''}: |y| {ny:.6e} |z| {nz:.6e} "
          f"error {err:.3e}")
    assert err < 1e-12 * ny
    mesh = po.BoxMesh(n)
    c = mesh.dof_coordinates(P)
    kq = 1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1]) + c[:, 2] if with_field else None
    T = tr.rotating_tensor(tr.cell_centres(mesh.xgeom, mesh.geom_dofmap))
    A = tr.with_tensor(tr.laplacian(P, 2.0, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, mesh.boundary_marker(P)),
                       T, kq)
    u = np.sin(1.0 + 3 * c[:, 0] + 5 * c[:, 1] * c[:, 2])
    assert abs(ny - np.linalg.norm(A.apply(u))) < 1e-12 * ny


def test_pmg_driver_converges(gpu):
    out = run("pmg_main", "--n", 16, "--orders", "1,2,4", "--amg", "--pcg", "--kappa-tensor")
    assert "AMG coarse solver:" in out
    m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
    print(m.group(0))
    assert int(m.group(1)) < 100 and float(m.group(2)) < 1e-6  # the driver's own limits: 100 iterations, rtol 1e-8
