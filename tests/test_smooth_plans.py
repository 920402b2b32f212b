"""The Chebyshev smooth's kernel sequence, checked on the host (no GPU).

``for_each_smooth_step`` (csrc/smooth_plan.hpp) decides which operator applications and vector passes a smoother call
issues, into which buffers, and what it leaves to its consumer; ``cheb_iterate`` (csrc/solvers.hip) only turns the
steps into launches.  A wrong sequence is a stale read or a residual nobody formed, which a parity test sees only on
the configuration that happens to take that path.  ``tests/host/smooth_check.cpp`` is a stand-alone program, compiled
host-only under the address and undefined-behaviour sanitizers with floating-point contraction off: it executes the
visitor's own steps on ``std::vector`` for the full product of a call's fields (k = 0 .. 5, the four residual modes,
x = 0, zeroed output, tracked ghosts, current ghosts, the recomputed form, double and float) on a small dense operator
with ghosts, and holds iterate and residual to the plain loop of src/chebyshev.hpp:46-91 with ``==``.  It is never
loaded into Python.

Each test runs one group in a subprocess and asserts exit status 0 and the coverage flags of its summary line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pmg-dolfinx_amd", "csrc")

# group -> (coverage flags its cases must reach, cases, refused calls, time limit in seconds).  Measured under the
# sanitizers on one core: fp64 0.13 s, fp32 0.06 s, the mutations 0.05 s, the list 0.01 s; a start of the sanitizer
# runtime on a busy machine is the larger part, so the limits are 5 s.
COMMON = ["k0", "one_step_none", "one_step_residual", "x_zero", "need_none", "need_updated", "need_split", "need_fused",
          "left_none", "left_split", "left_fused", "ghosts", "ghosts_current", "design_pass_counts"]
GROUPS = {
    "fp64": (COMMON + ["recomputed_k2", "recomputed_k3", "zeroed_output"], 768, 0, 5),
    # float: a zeroed-output operator or the recomputed form allowed is refused, 3 of every 4 calls of the product
    "fp32": (COMMON + ["float", "refused_zeroed", "refused_recompute"], 192, 576, 5),
}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not on this machine")
    exe = str(tmp_path_factory.mktemp("smooth_check") / "smooth_check")
    # (host code only: the sanitizer options are given to the host compilation alone, no device code is built)
    cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "smooth_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the checker does not compile:\n" + r.stderr[-4000:]
    return exe


def _run(exe, arg, limit):
    r = subprocess.run([exe, arg], capture_output=True, text=True, timeout=limit)
    return r.returncode, r.stdout + r.stderr


def _summary(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("SUMMARY ")]
    assert len(lines) == 1, out[-4000:]
    return dict(kv.split("=", 1) for kv in lines[0].split()[1:])


def test_groups_and_flags_are_the_checkers(checker):
    """The table above names exactly the checker's groups, and together its groups reach every flag it knows."""
    rc, out = _run(checker, "--list", 5)
    assert rc == 0, out
    lines = out.split()
    at = lines.index("FLAGS")
    assert sorted(lines[:at]) == sorted(GROUPS)
    reached = set()
    for flags, _, _, _ in GROUPS.values():
        reached |= set(flags)
    assert reached == set(lines[at + 1:])


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_smooth_schedules(checker, group):
    flags, cases, refused, limit = GROUPS[group]
    rc, out = _run(checker, group, limit)
    assert rc == 0, out[-6000:]
    s = _summary(out)
    assert s["group"] == group and s["violations"] == "0"
    # the full product: 6 step counts x 4 residual modes x 2^5 switches = 768 calls per scalar type
    assert int(s["cases"]) == cases and int(s["refused"]) == refused and cases + refused == 768
    reached = set(s["coverage"].split(",")) if s.get("coverage") else set()
    missing = [f for f in flags if f not in reached]
    assert not missing, f"no case of group {group} reached {missing}:\n{out[-3000:]}"


def test_mutated_schedules_are_reported(checker):
    """The checker can fail: every single corruption of a valid schedule is reported by what it computes."""
    rc, out = _run(checker, "--mutate", 5)
    assert rc == 0, out[-6000:]
    s = _summary(out)
    assert int(s["mutations"]) >= 10 and s["undetected"] == "0", out
    assert "FAIL" not in out
    for kind in ("dropped step", "swapped steps", "x_final set to 2", "clear_q dropped", "application output redirected"):
        assert kind in out, kind
