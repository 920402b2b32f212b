"""--form-gradients in the C++ mat_free driver (examples/mat_free, over include/pmg_amd.hpp): after the apply it prints the
three Euler sums of pmg_laplacian_form_gradients -- each coefficient of the diffusion term times its gradient, summed --
beside u_m . (A_diff v_m) of the apply, and their relative differences.  The four are one number computed by two
kernels, so the differences are rounding: at most 1e-12.  The driver runs as a separate process that links
libpmg_amd.so, each run under its own time limit."""
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


@pytest.mark.parametrize("extra", [("--kappa-field", "--kappa-tensor", "--reaction", "3"), ("--curved", "2")],
                         ids=lambda e: " ".join(e))
def test_form_gradients_option_agrees_with_the_apply(gpu, extra):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    r = subprocess.run([EXE, "--n", "4", "--degree", "3", "--nreps", "2", "--form-gradients", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    dot = float(re.search(r"Form gradients: u_m \. \(A_diff v_m\) = (\S+)", r.stdout).group(1))
    names = ["kappa", "field", "tensor"] + (["sigma"] if "--reaction" in extra else [])
    rel = {k: float(re.search(rf"Form gradients: relative difference \({k}\) = (\S+)", r.stdout).group(1))
           for k in names}
    print(f"mat_free_main --form-gradients {' '.join(extra)}: u_m . (A_diff v_m) = {dot:.15e}, rel. diff {rel}")
    assert dot != 0.0
    assert ("relative difference (sigma)" in r.stdout) == ("--reaction" in extra)
    for k in names:
        assert rel[k] <= 1e-12, (k, rel[k])
