"""--curved G in the C++ drivers (examples/, over include/pmg_amd.hpp): the box bent by the fixed smooth map of
examples/common/box_mesh.hpp and handed to the library with a coordinate element of degree G; the adapter infers G from
the geometry dofmap's width.  The drivers run as separate processes that link libpmg_amd.so."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import curved_geometry_reference as cg  # noqa: E402

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


def curved_map(x):
    return np.stack([x[:, 0] + 0.05 * np.sin(2.0 * x[:, 1] + x[:, 2]), x[:, 1] + 0.05 * np.sin(2.0 * x[:, 2] + x[:, 0]),
                     x[:, 2] + 0.05 * np.sin(2.0 * x[:, 0] + x[:, 1])], axis=1)


def test_mat_free_driver_against_csr_and_reference(gpu):
    """The matrix-free apply on the curved mesh against the driver's own assembled operator, at the bound its siblings
    apply to that comparison (1e-12 |y|), and |y| against the reference on the same mesh -- which is not the |y| of the
    straight-sided mesh through the same vertices."""
    import pmg_dolfinx_amd as pm

    n, P, g = 6, 3, 2
    out = run("mat_free_main", "--n", n, "--degree", P, "--curved", g, "--mat_comp", "--nreps", 3)
    assert f"coordinate element of degree {g}" in out
    (ny,) = grab(r"Norm of y = (\S+)", out)
    (nz,) = grab(r"Norm of z = (\S+)", out)
    (err,) = grab(r"Norm of error = (\S+)", out)
    print(f"mat_free_main --curved {g}: |y| {ny:.6e} |z| {nz:.6e} error {err:.3e}")
    assert err < 1e-12 * ny
    box = pm.BoxPartition(n)
    lv = box.level(P)
    norms = {}
    for gg in (1, g):
        x, gd = cg.box_mesh(n, gg, warp=curved_map)
        A = cg.laplacian(P, gg, 2.0, lv.dofmap, x, gd, lv.bc_marker)
        norms[gg] = np.linalg.norm(A.apply(np.ones(lv.ndofs)))  # the driver's u = 1
    assert abs(ny - norms[g]) < 1e-12 * ny
    assert abs(ny - norms[1]) > 1e-6 * ny
    (ny1,) = grab(r"Norm of y = (\S+)", run("mat_free_main", "--n", n, "--degree", P, "--curved", 1, "--nreps", 1))
    assert abs(ny1 - norms[1]) < 1e-12 * ny1


def test_pmg_driver_converges_as_on_the_straight_sided_mesh(gpu):
    its = {}
    for g in (1, 2):
        out = run("pmg_main", "--n", 8, "--orders", "1,2,4", "--curved", g, "--amg", "--pcg")
        assert "AMG coarse solver:" in out and f"coordinate element of degree {g}" in out
        m = re.search(r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = ([0-9.e+-]+)", out)
        print(f"pmg_main --curved {g}:", m.group(0))
        assert int(m.group(1)) < 100 and float(m.group(2)) < 1e-6  # the driver's own limits: 100 iterations, rtol 1e-8
        its[g] = int(m.group(1))
    assert abs(its[2] - its[1]) <= 1
