"""The renewal of an AMG hierarchy (csrc/amg_renew.hpp) checked on the CPU (no GPU).

The plan and the row routines of ``pmg_amg_update_values`` are free of HIP calls; the device kernels only call the
routines, a sub-wavefront per row.  ``tests/host/amg_update_check.cpp`` is a stand-alone program that includes the
header alone, compiled host-only under the address and undefined-behaviour sanitizers with floating-point contraction
off.  It reads a case this test writes -- a mesh, and the geometry tensor before and after a coefficient change (the
rotating tensor of the drivers, with a reaction vector) --, creates the hierarchy, plans, runs one update through the
row routines and writes every pattern and value.  The test compares with scipy: the patterns are the boolean products
of the structural definition (P_l from the entries of A_l that a coefficient can make non-zero, the products on the
stored patterns), the R permutation is a bijection with consistent columns, the values meet the
restatement of tests/test_gpu_amg_update.py at its tolerances, and one thread and three give the same bytes.  The
program also runs a hand-made matrix with a negative diagonal entry through the update, which must refuse its level,
and plans one with a row of 8200 entries, more than the kernels' row copy holds, which the plan must refuse.
It is never loaded into Python."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402
from oracle import amg_oracle as ao  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

CSRC = os.path.join(ROOT, "pmg-dolfinx_amd", "csrc")


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


# name: (cells, warp, level sizes, time limit of one run in seconds); the meshes of tests/test_amg_setup_host.py
CASES = {
    "two-layers": ((16, 16, 3), twist, [1156, 86], 10),
    "two-levels": (12, twist, [2197, 183], 10),
    "unwarped": (12, None, [2197, 183], 10),
    "row-blocks": (20, twist, [9261, 849, 103], 10),
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
    exe = str(tmp_path_factory.mktemp("amg_update_check") / "amg_update_check")
    # (host code only: the sanitizer options are given to the host compilation alone, no device code is built)
    cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "amg_update_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the checker does not compile:\n" + r.stderr[-4000:]
    return exe


def _read(blob):
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
    out = {"created": [matrix() for _ in range(L)], "A": [matrix() for _ in range(L)]}
    for name in ("P", "R", "AP"):
        out[name] = [matrix() for _ in range(L - 1)]
    out["perm"] = [take(np.int32, int(take(np.int32, 1)[0])) for _ in range(L - 1)]
    out["bound"] = take(np.float64, L)
    assert at == len(blob)
    return out


def pattern(M):
    """The stored positions of M as a sorted boolean CSR matrix (stored zeros count)."""
    B = sp.csr_matrix((np.ones(M.indices.size), M.indices.copy(), M.indptr.copy()), shape=M.shape)
    B.sort_indices()
    return B


def same_pattern(M, B):
    return np.array_equal(M.indptr, B.indptr) and np.array_equal(M.indices, B.indices)


def live_level0(A0, dofmap):
    """The stored entries of A_0 that some coefficient can make non-zero: the diagonal, and what two nodes i, j of a
    cell with i ^ j != 7 couple.  The 2-point GLL rule gives a gradient at point q to the nodes q, q ^ 1, q ^ 2 and
    q ^ 4 only, so no point couples the two ends of a cell's body diagonal, whatever the tensor."""
    n = A0.shape[0]
    pairs = [(i, j) for i in range(8) for j in range(8) if i ^ j != 7]
    rows = np.concatenate([dofmap[:, i] for i, _ in pairs] + [np.arange(n)])
    cols = np.concatenate([dofmap[:, j] for _, j in pairs] + [np.arange(n)])
    C = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    C.data[:] = 1.0
    L = pattern(A0).multiply(C).tocsr()
    L.eliminate_zeros()
    return pattern(L)


def structural_prolongator(live, agg, na):
    """(i, a) iff agg[i] >= 0 and (agg[i] = a, or some live stored (i, j) of A has agg[j] = a)."""
    n = live.shape[0]
    inside = agg >= 0
    rows = np.nonzero(inside)[0]
    T = sp.csr_matrix((np.ones(rows.size), (rows, agg[rows])), shape=(n, na))
    S = sp.diags(inside.astype(np.float64)) @ (T + live @ T)
    S = S.tocsr()
    S.sort_indices()
    return pattern(S)


class _Case:
    def __init__(self, exe, name, tmp):
        n, warp, self.sizes, limit = CASES[name]
        mesh = po.BoxMesh(n, warp=warp)
        self.bc = mesh.boundary_marker(1)
        self.dofmap = dofmap = np.ascontiguousarray(mesh.dofmap(1), dtype=np.int32)
        G0, _ = po.geometry_G(mesh.xgeom, mesh.geom_dofmap, *po.geometry_tables(1))
        T = tr.rotating_tensor(tr.cell_centres(mesh.xgeom, mesh.geom_dofmap))
        sigma = 3.0 * (1.0 + tr.cell_centres(mesh.xgeom, mesh.geom_dofmap)[:, 0])
        self.ref = tr.with_tensor(tr.laplacian(1, KAPPA, dofmap, mesh.xgeom, mesh.geom_dofmap, self.bc), T)
        d = rr.reaction_vector(1, sigma, dofmap, mesh.xgeom, mesh.geom_dofmap, self.bc)
        self.want0 = (self.ref.assemble_csr() + sp.diags(d)).tocsr()
        case = tmp / f"{name}.case"
        with open(case, "wb") as f:
            f.write(np.array([dofmap.shape[0], self.bc.size], dtype=np.int32).tobytes())
            f.write(dofmap.tobytes())
            f.write(self.bc.astype(np.int8).tobytes())
            f.write(np.full(dofmap.shape[0], KAPPA).tobytes())
            f.write(np.ascontiguousarray(G0, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(self.ref.G, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(d, dtype=np.float64).tobytes())
        self.blobs, self.said = [], []
        for threads in (1, 3):
            out = tmp / f"{name}.{threads}.out"
            r = subprocess.run([exe, str(case), str(out)], capture_output=True, text=True, timeout=limit,
                               env=dict(os.environ, PMG_HOST_THREADS=str(threads)))
            assert r.returncode == 0, f"PMG_HOST_THREADS={threads}:\n" + (r.stdout + r.stderr)[-6000:]
            self.said.append(r.stdout)
            self.blobs.append(out.read_bytes())
        self.h = _read(self.blobs[0])
        self.aggs = [ao.aggregate(A, 0.08 / 2 ** l) for l, A in enumerate(self.h["created"][:-1])]


_cache = {}


@pytest.fixture(scope="module")
def case(checker, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("amg_update_cases")

    def get(name):
        if name not in _cache:
            _cache[name] = _Case(checker, name, tmp)
        return _cache[name]

    return get


@pytest.mark.parametrize("name", list(CASES))
def test_update_does_not_depend_on_the_threads_and_the_hand_made_matrices_are_refused(case, name):
    c = case(name)
    assert c.blobs[0] == c.blobs[1]
    for threads, said in zip((1, 3), c.said):
        assert f"threads {threads} negative diagonal refused long row refused" in said and said.endswith("OK\n"), said


@pytest.mark.parametrize("name", list(CASES))
def test_patterns_are_the_structural_products(case, name):
    c = case(name)
    h = c.h
    assert [A.shape[0] for A in h["A"]] == c.sizes
    assert same_pattern(h["A"][0], pattern(h["created"][0]))
    live = live_level0(h["A"][0], c.dofmap)
    dead = h["A"][0] - h["A"][0].multiply(live)
    assert live.nnz < h["A"][0].nnz and abs(dead).max() == 0.0  # body diagonals: stored, and exact zeros
    for l, (agg, na) in enumerate(c.aggs):
        A, P, R, AP = h["A"][l], h["P"][l], h["R"][l], h["AP"][l]
        assert P.shape == (A.shape[0], na)
        assert same_pattern(P, structural_prolongator(live, agg, na))
        live = pattern((pattern(P).T @ (live @ pattern(P))).tocsr())
        Rt = pattern(P).T.tocsr()
        Rt.sort_indices()
        assert same_pattern(R, Rt)
        for got, (X, Y) in ((AP, (A, P)), (h["A"][l + 1], (R, AP))):
            want = (pattern(X) @ pattern(Y)).tocsr()
            want.sort_indices()
            assert same_pattern(got, want)
        # the structural patterns contain the created ones
        created = pattern(h["created"][l + 1])
        assert (pattern(h["A"][l + 1]) - created).min() >= 0
        if name != "unwarped":  # warped cells: every live entry is non-zero, the renewal changes no entry count
            assert h["A"][l + 1].nnz == h["created"][l + 1].nnz
    if name == "unwarped":  # the created P_0 stores no exact zero: the rotating tensor reaches further
        P0 = ao.smoothed_prolongator(h["created"][0], *c.aggs[0], 1.05 * ao.power_bound(h["created"][0]))
        P0.eliminate_zeros()
        assert h["P"][0].nnz > P0.nnz


@pytest.mark.parametrize("name", list(CASES))
def test_permutation_is_a_bijection_with_consistent_columns(case, name):
    h = case(name).h
    for P, R, perm in zip(h["P"], h["R"], h["perm"]):
        assert perm.size == P.nnz and np.array_equal(np.sort(perm), np.arange(P.nnz))
        prow = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        rrow = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
        assert np.array_equal(P.indices[perm], rrow) and np.array_equal(prow[perm], R.indices)
        assert np.array_equal(R.data, P.data[perm])


@pytest.mark.parametrize("name", list(CASES))
def test_values_equal_the_restatement(case, name):
    c = case(name)
    h = c.h
    assert abs(h["A"][0] - c.want0).max() < 1e-12 * abs(c.want0).max()
    for l, A in enumerate(h["A"]):
        bound = 1.05 * ao.power_bound(A)
        assert abs(h["bound"][l] - bound) <= 1e-11 * bound, (l, h["bound"][l], bound)
    for l, (agg, na) in enumerate(c.aggs):
        A, P = h["A"][l], h["P"][l]
        want = ao.smoothed_prolongator(A, agg, na, h["bound"][l])
        assert abs(P - want).max() <= 1e-13 * abs(want).max()
        AP = (A @ P).tocsr()
        assert abs(h["AP"][l] - AP).max() < 1e-12 * abs(AP).max()
        Ac = (P.T @ AP).tocsr()
        assert abs(h["A"][l + 1] - Ac).max() < 1e-12 * abs(Ac).max()
