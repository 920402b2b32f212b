"""The AMG host set-up (csrc/amg_setup.hpp) checked on the CPU (no GPU).

The set-up is plain C++ on ``std::vector`` -- threads, per-thread scratch, index arithmetic on gathered tables -- and
csrc/amg.hip only moves its inputs and results.  ``tests/host/amg_setup_check.cpp`` is a stand-alone program that
includes the header alone, compiled host-only under the address and undefined-behaviour sanitizers with floating-point
contraction off.  It reads a case this test writes, assembles level 0, runs the coarsening loop and writes every A_l,
P_l and bound; the test compares them with the restatements (``oracle/pmg_oracle.py``, ``oracle/amg_oracle.py``) to the
tolerances of tests/test_gpu_amg_setup.py, on that file's meshes.  The program also sends A_0 through both gathers
between two synthetic ranks and requires it back entry for entry.  It is never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import amg_oracle as ao
from oracle import pmg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pmg-dolfinx_amd", "csrc")


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def flat_twist(x):
    return twist(x) * np.array([1.0, 1.0, 0.04])


# name: (cells, warp, level sizes, time limit of one run in seconds).  One run measured under the sanitizers, with one
# thread and with three alike: two-layers 0.05 s, two-levels 0.07 s, flat 0.24 s, unwarped 0.07 s, row-blocks 0.27 s
# (9261 rows = three row blocks of the threaded loops); a start of the sanitizer runtime on a busy machine is the
# larger part, so the limits are 5 s.
CASES = {
    "two-layers": ((16, 16, 3), twist, [1156, 86], 5),
    "two-levels": (12, twist, [2197, 183], 5),
    "flat": (14, flat_twist, [3375, 845, 247], 5),
    "unwarped": (12, None, [2197, 183], 5),
    "row-blocks": (20, twist, [9261, 849, 103], 5),
}
KAPPA = 2.0


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
    exe = str(tmp_path_factory.mktemp("amg_setup_check") / "amg_setup_check")
    # (host code only: the sanitizer options are given to the host compilation alone, no device code is built)
    cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "amg_setup_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the checker does not compile:\n" + r.stderr[-4000:]
    return exe


def _read(blob):
    """(As, Ps, bounds) of the program's output."""
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(blob, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a

    def matrix():
        rows, cols, nnz = take(np.int32, 3)
        rp, ci, v = take(np.int32, rows + 1), take(np.int32, nnz), take(np.float64, nnz)
        return sp.csr_matrix((v, ci, rp), shape=(rows, cols))

    L = int(take(np.int32, 1)[0])
    As = [matrix() for _ in range(L)]
    Ps = [matrix() for _ in range(L - 1)]
    bounds = take(np.float64, L)
    assert at == len(blob)
    return As, Ps, bounds


class _Case:
    """One mesh: the program's hierarchy with one and with three threads, and the restated level 0 (shared by the
    tests, never modified)."""

    def __init__(self, exe, name, tmp):
        n, warp, self.sizes, limit = CASES[name]
        mesh = po.BoxMesh(n, warp=warp)
        self.bc = mesh.boundary_marker(1)
        dofmap = np.ascontiguousarray(mesh.dofmap(1), dtype=np.int32)
        G, _ = po.geometry_G(mesh.xgeom, mesh.geom_dofmap, *po.geometry_tables(1))
        case = tmp / f"{name}.case"
        with open(case, "wb") as f:
            f.write(np.array([dofmap.shape[0], self.bc.size], dtype=np.int32).tobytes())
            f.write(dofmap.tobytes())
            f.write(self.bc.astype(np.int8).tobytes())
            f.write(np.full(dofmap.shape[0], KAPPA).tobytes())
            f.write(np.ascontiguousarray(G, dtype=np.float64).tobytes())
        self.blobs, self.said = [], []
        for threads in (1, 3):
            out = tmp / f"{name}.{threads}.out"
            r = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=limit,
                               env=dict(os.environ, PMG_HOST_THREADS=str(threads)))
            assert r.returncode == 0, f"PMG_HOST_THREADS={threads}:\n" + (r.stdout + r.stderr)[-6000:]
            self.said.append(r.stdout)
            self.blobs.append(out.read_bytes())
        self.As, self.Ps, self.bounds = _read(self.blobs[0])
        self.ref = po.Laplacian(1, KAPPA, dofmap, mesh.xgeom, mesh.geom_dofmap, self.bc).assemble_csr()


_cache = {}


@pytest.fixture(scope="module")
def case(checker, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("amg_setup_cases")

    def get(name):
        if name not in _cache:
            _cache[name] = _Case(checker, name, tmp)
        return _cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_hierarchy_does_not_depend_on_the_threads_and_both_gathers_return_the_matrix(case, name):
    h = case(name)
    assert h.blobs[0] == h.blobs[1]
    for threads, said in zip((1, 3), h.said):
        assert f"threads {threads} slots back segments back" in said and said.endswith("OK\n"), said


@pytest.mark.parametrize("name", list(CASES))
def test_level_zero_and_level_sizes(case, name):
    h = case(name)
    assert abs(h.As[0] - h.ref).max() < 1e-12 * abs(h.ref).max()
    assert [A.shape[0] for A in h.As] == h.sizes
    if name == "row-blocks":
        assert h.sizes[0] > 2 * ao.ROW_BLOCK
    if name == "unwarped":
        assert (h.As[0].data == 0.0).sum() > h.As[0].shape[0]  # explicit zeros in A_0: the products keep them


@pytest.mark.parametrize("name", list(CASES))
def test_prolongators_equal_the_restatement(case, name):
    h = case(name)
    for l, (A, P) in enumerate(zip(h.As, h.Ps)):
        agg, na = ao.aggregate(A, 0.08 / 2 ** l)
        assert P.shape == (A.shape[0], na)
        want = ao.smoothed_prolongator(A, agg, na, h.bounds[l])
        assert abs(P - want).max() <= 1e-13 * abs(want).max()
        want.eliminate_zeros()
        want.sort_indices()
        assert (P.data != 0.0).all()  # no stored zero
        assert np.array_equal(P.indptr, want.indptr) and np.array_equal(P.indices, want.indices)


@pytest.mark.parametrize("name", list(CASES))
def test_levels_and_bounds_equal_the_restated_build(case, name):
    h = case(name)
    As, Ps, rhos, _ = ao.build(h.As[0])
    assert [A.shape[0] for A in As] == [A.shape[0] for A in h.As]
    for l, (A, want) in enumerate(zip(h.As, As)):
        assert abs(A - want).max() < 1e-12 * abs(A).max()
        bound = 1.05 * ao.power_bound(A)
        assert abs(h.bounds[l] - bound) <= 1e-11 * bound, (l, h.bounds[l], bound)
