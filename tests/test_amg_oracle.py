"""The restated AMG set-up of ``oracle/amg_oracle.py`` (test infrastructure for tests/test_gpu_amg_setup.py) checked on
its own, without a GPU: the generator of the power method's start vector against the C++ standard library's output
(tests/golden/mt_uniform_golden.json), and the defining properties of smoothed aggregation on the CPU oracle's
degree-1 matrix."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import amg_oracle as ao
from oracle import pmg_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def test_start_vector_generator_against_the_cxx_library():
    with open(os.path.join(HERE, "golden", "mt_uniform_golden.json")) as f:
        gold = json.load(f)
    v = ao.mt_uniform_half_one(gold["count"])
    assert v.min() >= 0.5 and v.max() < 1.0
    for i, want in gold["values"].items():
        assert v[int(i)] == float(want), (i, v[int(i)], want)  # bit for bit
    s = 0.0
    for x in v.tolist():  # the same running sum as the program that wrote the fixture
        s += x
    assert s == float(gold["sum"])
    # the values the issue that introduced this file quotes
    assert v[:5].tolist() == [0.67881486144421299, 0.70022130852203057, 0.84469165850138417, 0.77986778532055778,
                              0.7872256469958554]


def test_hashed_start_is_the_64_bit_mix():
    M = (1 << 64) - 1
    g = np.array([0, 1, 2, 17, 1376, 15624, 2**31 - 1])
    got = ao.hashed_start(g)
    for gi, x in zip(g.tolist(), got.tolist()):
        h = (gi * 0x9E3779B97F4A7C15) & M
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & M
        h ^= h >> 32
        assert x == 0.5 + 0.5 * float(h >> 11) / 2.0 ** 53
        assert 0.5 <= x < 1.0


@pytest.fixture(scope="module")
def problem():
    n = 10
    mesh = po.BoxMesh(n, warp=twist)
    bc = mesh.boundary_marker(1).astype(bool)
    dofmap = np.asarray(mesh.dofmap(1)).reshape(-1, 8)
    A = po.Laplacian(1, 2.0, dofmap, mesh.xgeom, mesh.geom_dofmap, bc).assemble_csr()
    near_bc = np.zeros(bc.size, bool)  # dofs that share a cell with a Dirichlet dof
    near_bc[dofmap[bc[dofmap].any(axis=1)].ravel()] = True
    return A, bc, near_bc


def _lambda_true(A):
    d = A.diagonal()
    return float(np.linalg.eigvalsh(A.toarray() / np.sqrt(np.outer(d, d)))[-1])  # D^-1 A ~ D^-1/2 A D^-1/2


def test_restated_setup_has_the_defining_properties(problem):
    A, bc, near_bc = problem
    stats = {}
    agg, na = ao.aggregate(A, 0.08, stats)
    # the aggregates partition the non-Dirichlet rows: every such row in exactly one, numbered 0 .. na - 1, none empty
    assert np.array_equal(agg >= 0, ~bc)
    assert agg.max() == na - 1 and np.bincount(agg[agg >= 0], minlength=na).min() >= 1
    assert stats["pass1_roots"] + stats["pass3_roots"] == na and stats["outside"] == bc.sum()
    assert 0.03 * (~bc).sum() < na < 0.35 * (~bc).sum()  # real coarsening
    lam = ao.power_bound(A)
    lam_true = _lambda_true(A)
    print(f"power_bound / lambda_max(D^-1 A) = {lam / lam_true:.4f}")
    assert 0.0 < lam <= lam_true
    rho = 1.05 * lam
    P = ao.smoothed_prolongator(A, agg, na, rho)
    assert P.shape == (A.shape[0], na) and abs(P[bc]).sum() == 0.0
    # the definition, densely: P = (I - 4 / (3 rho) D^-1 A) T, T[i, agg[i]] = 1 / sqrt(size)
    size = np.bincount(agg[agg >= 0], minlength=na)
    T = np.zeros(P.shape)
    T[np.nonzero(~bc)[0], agg[~bc]] = 1.0 / np.sqrt(size[agg[~bc]])
    want = T - (4.0 / (3.0 * rho)) * (A.toarray() @ T) / A.diagonal()[:, None]
    want[bc] = 0.0
    assert np.abs(P.toarray() - want).max() < 1e-14
    # P (T^T 1) = (I - omega D^-1 A) 1 = 1 where A 1 = 0: on the rows with no Dirichlet neighbour
    c = np.asarray(sp.csr_matrix(T).T @ np.ones(A.shape[0])).ravel()
    assert np.allclose(c, np.sqrt(size), rtol=1e-14)
    Pc = P @ c
    assert (~near_bc).sum() > 100
    assert np.abs(Pc[~near_bc] - 1.0).max() < 1e-12
    assert np.abs(Pc[near_bc & ~bc] - 1.0).max() > 1e-3  # ... and only there
    # the Galerkin operator is symmetric positive definite
    Ac = (P.T @ A @ P).toarray()
    assert np.abs(Ac - Ac.T).max() < 1e-12 * np.abs(Ac).max()
    assert np.linalg.eigvalsh(0.5 * (Ac + Ac.T)).min() > 0.0


def test_build_stops_as_stated_and_uses_its_own_bounds(problem):
    A, bc, _ = problem
    As, Ps, rhos, stats = ao.build(A)
    assert [M.shape[0] for M in As] == [A.shape[0], stats[0]["pass1_roots"] + stats[0]["pass3_roots"]]
    assert As[-1].shape[0] <= 800 and len(Ps) == 1 and len(rhos) == 2
    for M, rho in zip(As, rhos):
        assert rho == 1.05 * ao.power_bound(M)
    agg, na = ao.aggregate(A, 0.08)
    assert abs(Ps[0] - ao.smoothed_prolongator(A, agg, na, rhos[0])).max() == 0.0
    assert abs(As[1] - Ps[0].T @ A @ Ps[0]).max() < 1e-13 * abs(As[1]).max()
    # a lower ceiling: one more coarsening, at half the threshold
    As3, Ps3, rhos3, stats3 = ao.build(A, coarsest_max=50)
    assert len(As3) >= 3 and As3[1].shape == As[1].shape and As3[-1].shape[0] <= 50
    agg1, na1 = ao.aggregate(As3[1], 0.04)
    assert na1 == As3[2].shape[0]
    assert abs(Ps3[1] - ao.smoothed_prolongator(As3[1], agg1, na1, rhos3[1])).max() == 0.0
    # nothing larger than the ceiling: no coarsening at all; the level limit stops it too
    one = ao.build(As[1])
    assert len(one[0]) == 1 and len(one[1]) == 0 and len(one[2]) == 1
    assert len(ao.build(A, coarsest_max=1, max_levels=2)[0]) == 2


def test_the_three_passes_on_crafted_matrices():
    # a chain 0 - 1 - 2 - 3 - 4 with couplings 1, 1, 3, 3: pass 1 makes {0, 1} (root 0) and {3, 2, 4} (root 3)
    def chain(w):
        n = len(w) + 1
        A = np.diag(np.full(n, 10.0))
        for i, x in enumerate(w):
            A[i, i + 1] = A[i + 1, i] = -x
        return sp.csr_matrix(A)

    st = {}
    agg, na = ao.aggregate(chain([1, 1, 3, 3]), 0.05, st)
    assert agg.tolist() == [0, 0, 1, 1, 1] and na == 2 and st["pass3_roots"] == 0
    # the threshold: theta sqrt(10 * 10) = 1 keeps a coupling of exactly 1, anything above drops it
    agg, na = ao.aggregate(chain([1, 1, 3, 3]), 0.1)
    assert agg.tolist() == [0, 0, 1, 1, 1]
    agg, na = ao.aggregate(chain([1, 1, 3, 3]), 0.1000001)
    assert agg.tolist() == [-1, -1, 0, 0, 0] and na == 1
    # pass 2: roots 0 and 3 take {0, 1} and {3, 2, 4}; 5 is tied to 1 (aggregate 0) and to 4 (aggregate 1):
    # the strictly stronger coupling wins, and of two equal ones the first in the row
    def ring(w15, w45):
        A = chain([1, 1, 1, 1]).toarray()
        A = np.pad(A, (0, 1))
        A[5, 5] = 10.0
        A[1, 5] = A[5, 1] = -w15
        A[4, 5] = A[5, 4] = -w45
        return sp.csr_matrix(A)

    assert ao.aggregate(ring(2, 3), 0.05)[0].tolist() == [0, 0, 1, 1, 1, 1]
    assert ao.aggregate(ring(3, 2), 0.05)[0].tolist() == [0, 0, 1, 1, 1, 0]
    assert ao.aggregate(ring(2, 2), 0.05)[0].tolist() == [0, 0, 1, 1, 1, 0]  # a tie: column 1 comes before column 4
    # pass 3 needs a strength graph that is not symmetric (with a symmetric one, a row that pass 1 passes over has a
    # strong neighbour in a pass-1 aggregate, which pass 2 then joins): row 0 sees 1 and 2, they see nobody (outside),
    # so row 0 is no root in pass 1, finds no aggregate in pass 2 and is left to pass 3
    A = sp.csr_matrix(np.array([[10.0, -5.0, -5.0], [-0.1, 10.0, 0.0], [-0.1, 0.0, 10.0]]))
    st = {}
    agg, na = ao.aggregate(A, 0.08, st)
    assert agg.tolist() == [0, -1, -1] and na == 1 and st == {"pass1_roots": 0, "pass3_roots": 1, "outside": 2}


def test_stationary_cycles_of_the_restated_solve(problem):
    A, bc, _ = problem
    As, Ps, rhos, _ = ao.build(A)
    ref = ao.AmgCycle(As, Ps, rhos, 2)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    b[bc] = 0.0
    xs = np.linalg.solve(A.toarray(), b)
    x1, x3 = ref.stationary(b, 1), ref.stationary(b, 3)
    assert np.array_equal(x1, ref.cycle(b))
    e1, e3 = np.abs(x1 - xs).max(), np.abs(x3 - xs).max()
    assert e3 < 0.2 * e1  # three cycles: the error contracts
    # x_3 = x_2 + M (b - A x_2)
    x2 = ref.stationary(b, 2)
    assert np.abs(x3 - (x2 + ref.cycle(b - A @ x2))).max() < 1e-14 * np.abs(x3).max()
