"""--cell-form in the C++ mat_free driver (examples/mat_free, over include/pmg_amd.hpp): after the apply y = A u it prints
the sum over the cells of e_c(u, u) (kappa, marked dofs read as zero) beside u_m . y and their relative difference.  The
two are one number computed by two kernels -- the cell form and the apply -- so the difference is rounding: below 1e-12.
The driver runs as a separate process that links libpmg_amd.so, each run under its own time limit."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pmg-dolfinx_amd", "bin", "mat_free_main")


@pytest.fixture(scope="module")
def gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("extra", [(), ("--kappa-tensor",), ("--curved", "2"), ("--kappa-tensor", "--curved", "2"),
                                   ("--kappa-field", "--kappa-tensor")], ids=lambda e: " ".join(e) or "plain")
def test_cell_form_option_agrees_with_the_apply(gpu, extra):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    r = subprocess.run([EXE, "--n", "4", "--degree", "3", "--nreps", "2", "--cell-form", *extra], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    energy = float(re.search(r"Cell form: sum_c e_c\(u, u\) = (\S+)", r.stdout).group(1))
    dot = float(re.search(r"Cell form: u_m \. y = (\S+)", r.stdout).group(1))
    rel = float(re.search(r"Cell form: relative difference = (\S+)", r.stdout).group(1))
    print(f"mat_free_main --cell-form {' '.join(extra)}: energy {energy:.15e} u_m.y {dot:.15e} rel. diff {rel:.3e}")
    assert energy > 0 and dot > 0
    assert rel < 1e-12


def test_without_the_option_nothing_is_printed(gpu):
    r = subprocess.run([EXE, "--n", "4", "--degree", "3", "--nreps", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Cell form" not in r.stdout
