"""The host pattern of the assembled operator and its diag / off-diag split (csrc/matrix_pattern.hpp) checked on the
CPU (no GPU).

``tests/host/matrix_pattern_check.cpp`` is a stand-alone program that includes the header alone, compiled host-only
under the address and undefined-behaviour sanitizers, the way tests/test_amg_setup_host.py builds its checker.  For every rank
of the partitions below this test writes the rank's ``BoxPartition`` level -- dofmap, applied cells, size_local,
num_ghosts --, the program builds the pattern and the split and runs the two-phase product serially on small integers
(exact, so "equal" means equal), and the test compares the arrays with the oracle's global pattern -- the (row, column)
pairs ``Laplacian.assemble_csr`` assembles into -- restricted to the rank's rows and renumbered through
``local_to_global``.  The program is never loaded into Python.

The partitions are the ones of tests/test_gpu_matrix_distributed.py, taken from ``SWEEP_CASES``
(tests/test_partition_shapes.py pins what the partitioner makes of them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pmg_oracle as po
from pmg_dolfinx_amd.mesh import BoxPartition
from test_partition_shapes import PREMISES, SWEEP_CASES, rank_facts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pmg-dolfinx_amd", "csrc")

CASES = [((1, 1, 3), (3, 3, 4), (1, 3, 6)),
         ((1, 1, 4), (3, 4, 4), (1, 2, 4)),
         ((2, 3, 1), (3, 4, 4), (1, 2)),
         ((2, 2, 2), (2, 2, 2), (2, 4))]
RUN_SECONDS = 20  # one rank's level: the largest (degree 6, 4332 rows of up to 2197 columns) runs in about a second


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
    exe = str(tmp_path_factory.mktemp("matrix_pattern_check") / "matrix_pattern_check")
    # (host code only: the sanitizer options are given to the host compilation alone, no device code is built)
    cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "matrix_pattern_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the checker does not compile:\n" + r.stderr[-4000:]
    return exe


def test_the_cases_are_sweep_cases():
    assert all(c in SWEEP_CASES for c in CASES)


def global_pattern(n, P):
    """The oracle's pattern as a CSR matrix of ones: the pairs Laplacian.assemble_csr assembles into, BC rows and
    columns included (they stay as explicit zeros)."""
    dm = np.asarray(po.BoxMesh(n).dofmap(P), dtype=np.int64)
    N = dm.shape[1]
    rows, cols = np.repeat(dm, N, axis=1).ravel(), np.tile(dm, (1, N)).ravel()
    nd = int(dm.max()) + 1
    A = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(nd, nd)).tocsr()  # duplicates summed
    A.sort_indices()
    return A


def restricted_pattern(G, lv):
    """(row_ptr, cols) of the rank's rows of G in the rank's numbering, columns sorted."""
    nl, l2g = lv.size_local, np.asarray(lv.local_to_global)
    inv = np.full(G.shape[0], -1, dtype=np.int64)
    inv[l2g] = np.arange(l2g.size)
    S = G[l2g[:nl]].tocsr()
    cols = inv[S.indices]
    assert (cols >= 0).all()  # the ghost-cell layer: every owned row is complete on its rank
    R = sp.csr_matrix((np.ones(cols.size), cols, S.indptr), shape=(nl, l2g.size))
    R.sort_indices()
    return R.indptr.astype(np.int32), R.indices.astype(np.int32)


def _read(blob):
    at = 0

    def take(count):
        nonlocal at
        a = np.frombuffer(blob, dtype=np.int32, count=count, offset=at)
        at += a.nbytes
        return a

    n, ncols, nnz, nb = (int(v) for v in take(4))
    out = {"n": n, "ncols": ncols, "rp": take(n + 1), "ci": take(nnz), "od": take(n), "brows": take(nb),
           "inc_off": take(n + 1)}
    assert at == len(blob)
    return out


_cache = {}


def run_rank(exe, tmp, dims, n, P, rank):
    key = (dims, n, P, rank)
    if key not in _cache:
        lv = BoxPartition(n, dims, rank).level(P)
        applied = np.sort(np.concatenate([lv.lcells, lv.bcells])).astype(np.int32)  # what the operator applies
        assert np.array_equal(applied, np.arange(lv.dofmap.shape[0]))               # ... ghost cells included
        name = "-".join(str(v) for v in dims + n + (P, rank))
        case, out = tmp / (name + ".case"), tmp / (name + ".out")
        with open(case, "wb") as f:
            f.write(np.array([lv.dofmap.shape[0], lv.dofmap.shape[1], lv.size_local, lv.num_ghosts, applied.size],
                             dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(lv.dofmap, dtype=np.int32).tobytes())
            f.write(applied.tobytes())
        r = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=RUN_SECONDS)
        assert r.returncode == 0 and r.stdout.endswith("OK\n"), (key, (r.stdout + r.stderr)[-4000:])
        _cache[key] = (lv, _read(out.read_bytes()))
    return _cache[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("matrix_pattern_cases")


@pytest.mark.parametrize("dims,n,orders", CASES, ids=[f"dims{i}" for i in range(len(CASES))])
def test_pattern_split_and_exact_product_on_every_rank(checker, tmp, dims, n, orders):
    """The program has run its own exact comparison of the two-phase product with the one-pass product (exit status);
    here its arrays against the oracle's pattern."""
    for P in orders:
        G = global_pattern(n, P)
        for rank in range(int(np.prod(dims))):
            lv, got = run_rank(checker, tmp, dims, n, P, rank)
            nl = lv.size_local
            assert (got["n"], got["ncols"]) == (nl, lv.ndofs)
            rp, ci = restricted_pattern(G, lv)
            assert np.array_equal(got["rp"], rp), (P, rank)
            assert np.array_equal(got["ci"], ci), (P, rank)
            # the split: the first column >= size_local of every row, entry for entry
            ghost = ci >= nl
            before = np.concatenate([[0], np.cumsum(~ghost)])
            od = rp[:-1] + (before[rp[1:]] - before[rp[:-1]])  # sorted rows: the owned columns come first
            assert np.array_equal(got["od"], od.astype(np.int32)), (P, rank)
            assert nl > 0 and (np.diff(rp) > 0).all()  # every row holds its diagonal: reduceat sees no empty row
            has_ghost = np.add.reduceat(ghost.astype(np.int64), rp[:-1])
            assert np.array_equal(got["brows"], np.flatnonzero(has_ghost > 0).astype(np.int32)), (P, rank)
            # incidences for owned rows only: one per (cell, node) that holds an owned dof
            assert got["inc_off"][-1] == int((lv.dofmap < nl).sum())


def test_the_case_set_has_the_ranks_the_split_can_go_wrong_on(checker, tmp):
    """Premises (tests/test_partition_shapes.py pins the partitioner's side of them)."""
    all_boundary_or_dirichlet = both = False
    for dims, n, orders in CASES:
        for P in orders:
            for rank in range(int(np.prod(dims))):
                lv, got = run_rank(checker, tmp, dims, n, P, rank)
                bc = lv.bc_marker[: lv.size_local].astype(bool)
                boundary = np.zeros(lv.size_local, dtype=bool)
                boundary[got["brows"]] = True
                all_boundary_or_dirichlet |= bool(lv.size_local > 0 and (boundary | bc).all() and boundary.any())
                both |= bool(boundary.any() and (~boundary & ~bc).any())
    assert all_boundary_or_dirichlet  # a rank on which every owned row is a boundary row or a Dirichlet row
    assert both                       # a rank with interior (free, ghost-free) rows and boundary rows
    assert all(f[3] == 7 for f in rank_facts((2, 2, 2), (2, 2, 2), 2))  # seven neighbours
    assert PREMISES[((1, 1, 4), (3, 4, 4))][2] == [3]                   # rank 3 owns no free degree-1 dof
    assert rank_facts((1, 1, 4), (3, 4, 4), 1)[3][1] == 0
