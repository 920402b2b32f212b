"""The launch plans the kernels trust blindly, checked on the host (no GPU).

``build_patch_plan``, ``build_chain_plan`` and ``build_coarse_plan`` (csrc/patches.hip) decide which patch writes a
dof first, which launches may store without atomics and what has to be zero beforehand.  A wrong list is a data race
on the device, which a parity test sees only when the race happens to lose.  ``tests/host/plan_check.cpp`` is a
stand-alone program, compiled host-only together with patches.hip under the address and undefined-behaviour
sanitizers: it builds plans for meshes it generates, checks every structural invariant and executes every schedule
serially in exact integer arithmetic against the cell-by-cell scatter-add.  The schedule it executes is the library's:
the steps come from the function the operator's apply walks (patches.hpp ``for_each_launch_step``), not from a model
of it.  It is never loaded into Python.

Each test runs one group of cases in a subprocess and asserts exit status 0 and the coverage flags of the group's
summary line, so a case that silently stops reaching a path fails."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pmg-dolfinx_amd", "csrc")

# group -> (coverage flags its cases must reach, time limit in seconds).  Measured under the sanitizers on one core: boxes
# 0.5 s, permuted 0.3, irregular 0.2, lists 0.7, coloured 0.6, split 2.2, chains 1.1, chains_production 3.5, transfers
# 0.8, the mutations 0.8; the limits are a few times that.  The form_* flags: every plan is executed as the library's
# own schedule (patches.hpp for_each_launch_step) yields it -- as the two calls of an application, as one whole walk
# (coalesced_step: a walk that merges contiguous atomic launches was reached), as the FP32 apply walks a split plan
# (fp32_unsplit), and in chain form.
WALKS = ["form_two_calls", "form_whole"]
GROUPS = {
    "boxes": (["tensor_grouping", "ragged_blocks", "below_one_patch", "single_cell_patch", "merged_interior",
               "coloured_interior", "interior_only", "boundary_only", "zero_all_rule", "bzero_list_rule"] + WALKS, 10),
    "permuted": (["ragged_blocks", "merged_interior", "coloured_interior", "interior_only", "coalesced_step"] + WALKS,
                 10),
    "irregular": (["morton_grouping", "halved_group", "halved_group_high_degree", "merged_interior",
                   "coloured_interior", "boundary_only", "coalesced_step"] + WALKS, 10),
    "lists": (["boundary_only", "interior_only", "empty_plan", "merged_interior", "coloured_interior",
               "coalesced_step"] + WALKS, 10),
    "coloured": (["coloured_interior", "tensor_grouping"] + WALKS, 10),
    "split": (["split_plan", "split_refused", "split_refused_colours", "coloured_interior", "fp32_unsplit"] + WALKS,
              10),
    "chains": (["chain_ok", "chain_refused_merged", "chain_refused_split", "chain_refused_grid",
                "chain_refused_colours", "chain_refused_few_chains", "form_chains"] + WALKS, 10),
    "chains_production": (["chain_ok", "form_chains"] + WALKS, 20),
    "transfers": (["coarse_coloured", "coarse_merged", "coarse_refused", "coalesced_step"] + WALKS, 10),
    # Meshes that are no boxes (stars of 3 and 5 sectors, the O-grid, the notched grid; 6.5 s).  The grouping flags are
    # required; the split, chain and coarse flags are what the builder yields there: the notched grid (a tensor grid of
    # centroids with gaps: tensor_grouping, ragged_blocks) is split over two streams, a star or an O-grid is not (the
    # colours of Morton patches do not separate the halves); no such mesh gets chains (its patches form no tensor
    # grid, or the level is merged or split) and each then runs, and is checked, in the patch form; every coarse plan
    # is accepted, coloured and merged.
    "multiblock": (["morton_grouping", "halved_group", "halved_group_high_degree", "coloured_interior",
                    "merged_interior", "coalesced_step", "tensor_grouping", "ragged_blocks", "split_plan",
                    "split_refused_colours", "fp32_unsplit", "chain_refused_grid", "chain_refused_merged",
                    "chain_refused_split", "coarse_coloured", "coarse_merged"] + WALKS, 40),
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
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check")
    # (host code only: the sanitizer options are given to the host compilation alone, no device code is built)
    cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
           "-I", os.path.join(ROOT, "examples", "common"),
           os.path.join(CSRC, "patches.hip"), os.path.join(ROOT, "tests", "host", "plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the checker does not compile:\n" + r.stderr[-4000:]
    return exe


def _run(exe, arg, limit):
    env = dict(os.environ)
    for k in ("PMG_APPLY_STREAMS", "PMG_CHAIN"):
        env.pop(k, None)  # (the checker sets what it needs itself)
    r = subprocess.run([exe, arg], capture_output=True, text=True, timeout=limit, env=env)
    return r.returncode, r.stdout + r.stderr


def _summary(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("SUMMARY ")]
    assert len(lines) == 1, out[-4000:]
    return dict(kv.split("=", 1) for kv in lines[0].split()[1:])


def test_groups_and_flags_are_the_checkers(checker):
    """The table above names exactly the checker's groups, and only flags it knows."""
    rc, out = _run(checker, "--list", 10)
    assert rc == 0, out
    lines = out.split()
    at = lines.index("FLAGS")
    assert sorted(lines[:at]) == sorted(GROUPS)
    known = set(lines[at + 1:])
    for flags, _ in GROUPS.values():
        assert set(flags) <= known


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_plans(checker, group):
    flags, limit = GROUPS[group]
    rc, out = _run(checker, group, limit)
    assert rc == 0, out[-6000:]
    s = _summary(out)
    assert s["group"] == group and int(s["cases"]) > 0 and s["violations"] == "0"
    reached = set(s["coverage"].split(",")) if s.get("coverage") else set()
    missing = [f for f in flags if f not in reached]
    assert not missing, f"no case of group {group} reached {missing}:\n{out[-3000:]}"


def test_every_listed_path_is_reached(checker):
    """Over all groups together: every path the checker reports, except an empty launch inside a split plan, which no
    generated mesh produces (each half of a tensor grid of patches has as many colours as the other)."""
    reached = set()
    for flags, _ in GROUPS.values():
        reached |= set(flags)
    rc, out = _run(checker, "--list", 10)
    assert rc == 0
    known = set(out.split()[out.split().index("FLAGS") + 1:])
    assert known - reached <= {"empty_launch_in_split"}, sorted(known - reached)


def test_mutated_plans_are_reported(checker):
    """The checker can fail: every single corruption of a valid plan is reported as a violation."""
    rc, out = _run(checker, "--mutate", 10)
    assert rc == 0, out[-6000:]
    s = _summary(out)
    assert int(s["mutations"]) >= 12 and s["undetected"] == "0", out
    assert "FAIL" not in out
