"""The multi-rank path on the partitions the equal-brick tests of tests/test_gpu_distributed.py leave out: bricks one
cell thick (a rank whose owned cells all touch the ghost plane has no interior cell list and takes the split form of an
operator application next to a neighbour that takes the one-launch form), neighbours with traffic in one direction
only (the ghost cell of the rank two bricks away reaches one plane into this rank's dofs), ranks that own no free
degree-1 dof, and uneven cuts.  tests/test_partition_shapes.py pins these premises on the host.

Part A: every shape with the ranks as threads of this process (exchange and all-reduce through the callbacks of the
C ABI), every rank's results compared with the single-domain oracle.  Part B: the thin chains with the ranks as
processes that exchange through the halo windows, eager and replayed as a hipGraph -- the pair of ranks that take
different forms of an application meet on the same window flags.

Bounds: tests/test_gpu_distributed.py (_assert_rank_results, _native_worker_body) and
tests/test_gpu_parity.py::test_transfer_parity."""
import threading
import time

import numpy as np
import pytest

from rank_harness import _run_ranks, _ThreadComm, _ThreadWorld
from test_gpu_distributed import _worker, warp
from test_partition_shapes import PREMISES, SWEEP_CASES, WINDOW_CASES, rank_facts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 3                 # Chebyshev iterations per smooth
BARRIER_SECONDS = 60  # the meshes are tiny: a rank that returned early fails the test quickly


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _ghost_value(global_dofs, rank):
    """What rank `rank` holds in its ghost copy of a dof before a reverse scatter: small integers, so every sum of them
    is exact whatever the order of the additions."""
    return ((np.asarray(global_dofs) * 7 + 13 * rank) % 11 - 5).astype(np.float64)


def _stale(lv, ug):
    """The rank's part of the global vector `ug` with its ghost entries not yet received."""
    xl = np.zeros(lv.ndofs)
    xl[: lv.size_local] = ug[lv.local_to_global[: lv.size_local]]
    return xl


def _vector(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _rank_body(pm, rank, world, n, dims, orders, comm, inputs):
    """What one rank computes on the device; nothing is judged here (a rank that failed a check of its own would
    leave the others waiting in the next collective)."""
    H = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=K, proc_dims=dims, rank=rank, size=world, warp=warp,
                            comm=comm)
    out = {"eig": H.eig_ranges,
           "l2g": [np.array(lv.local_to_global) for lv in H.levels],
           "owned": [lv.size_local for lv in H.levels],
           "cell_lists": [(len(lv.lcells), len(lv.bcells)) for lv in H.levels],
           "launches": [op.launches_per_apply() for op in H.operators],
           "apply": [], "input_after": [], "dot": [], "linf": [], "rev": [], "dinv": [], "prolong": [], "restrict": []}
    for i, (lv, layout, op) in enumerate(zip(H.levels, H.layouts, H.operators)):
        nl = lv.size_local
        x, y = _vector(pm, layout, _stale(lv, inputs["u"][i])), pm.Vector(layout)
        y.set(9.0)
        op(x, y)
        out["apply"].append(y.data_copy()[:nl].copy())
        out["input_after"].append(x.data_copy().copy())
        out["dot"].append(pm.inner_product(x, x))
        out["linf"].append(pm.norm(x, "linf"))
        # reverse scatter: the ghost copies are added into their owners
        loc = inputs["w"][i][lv.local_to_global].copy()
        loc[nl:] = _ghost_value(lv.local_to_global[nl:], rank)
        v = _vector(pm, layout, loc)
        v.scatter_rev()
        out["rev"].append(v.data_copy()[:nl].copy())
        d = pm.Vector(layout)
        op.get_diag_inverse(d)
        out["dinv"].append(d.data_copy()[:nl].copy())
    for i, ip in enumerate(H.interpolators):
        lc, lf = H.levels[i], H.levels[i + 1]
        vc, vf = _vector(pm, H.layouts[i], _stale(lc, inputs["u"][i])), pm.Vector(H.layouts[i + 1])
        vf.set(7.0)
        ip.interpolate(vc, vf)
        out["prolong"].append(vf.data_copy()[: lf.size_local].copy())
        vf2, vc2 = _vector(pm, H.layouts[i + 1], _stale(lf, inputs["u"][i + 1])), pm.Vector(H.layouts[i])
        vc2.set(3.0)  # must be zeroed by the restriction
        ip.reverse_interpolate(vf2, vc2)
        out["restrict"].append(vc2.data_copy()[: lc.size_local].copy())
    # two V-cycles, then the exchanges of one eager cycle
    nf = H.levels[-1].size_local
    xv = H.new_vector()
    xv.set(0.0)
    out["cycles"], out["rnorms"] = [], []
    for _ in range(2):
        out["rnorms"].append(H.mg.apply(H.rhs[-1], xv, verbose=True))
        out["cycles"].append(xv.data_copy()[:nf].copy())
    H.mg.set_graph(False)  # a replayed cycle issues its scatters once, at capture
    before = sum(l.forward_scatters() for l in H.layouts)
    H.mg.apply(H.rhs[-1], xv)
    H.mg.set_graph(None)
    out["exchanges"] = sum(l.forward_scatters() for l in H.layouts) - before
    # CG preconditioned by the cycle
    cg = pm.CGSolver(H.layouts[-1])
    cg.set_max_iterations(30)
    cg.set_tolerance(1e-9)
    xs = H.new_vector()
    xs.set(0.0)
    out["pcg_its"] = cg.solve(H.operators[-1], xs, H.rhs[-1], preconditioner=H.mg)
    out["pcg"] = xs.data_copy()[:nf].copy()
    if orders[0] != 1:
        return out
    # the degree-1 level: the three forms of the AMG over all ranks, and the rank-local one as coarse solver
    lv0, op0, lay0 = H.levels[0], H.operators[0], H.layouts[0]
    n0, N0 = lv0.size_local, H.part.global_ndofs(1)
    bl = _vector(pm, lay0, inputs["g"][lv0.local_to_global])
    for name, kw in (("rep", {}), ("rep_full", {"distributed_fine_level": False}), ("dis", {"setup": "distributed"})):
        amg = pm.AmgSolver(op0, max_iter=60, rtol=1e-9, global_index=lv0.local_to_global, n_global=N0, **kw)
        xl = pm.Vector(lay0)
        out[name + "_its"] = amg.solve(xl, bl)
        out[name] = xl.data_copy()[:n0].copy()
        out[name + "_levels"] = amg.info()
        del amg, xl
    amg = pm.AmgSolver(op0, max_iter=100, rtol=1e-11)
    H.mg.set_coarse_solver(amg)
    xv.set(0.0)
    out["amg_cycles"] = []
    for _ in range(2):
        H.mg.apply(H.rhs[-1], xv)
        out["amg_cycles"].append(xv.data_copy()[:nf].copy())
    H.mg.set_coarse_solver(None)
    return out


def _run_as_threads(pm, n, dims, orders, inputs):
    world = int(np.prod(dims))
    W = _ThreadWorld(world, barrier_timeout=BARRIER_SECONDS)
    res, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                res[rank] = _rank_body(pm, rank, world, n, dims, orders, _ThreadComm(W, rank), inputs)
                torch.cuda.current_stream().synchronize()
        except BaseException:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            W.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, "\n".join(f"rank {r}:\n{tb}" for r, tb in sorted(errors))
    assert all(r is not None for r in res)
    return res


def _maxrel(parts, ref):
    return max(float(np.abs(a - b).max()) for a, b in parts) / max(float(np.abs(ref).max()), 1e-300)


def _owned(res, get, level, ref):
    """(rank's owned values of level `level`, the oracle's at the same dofs) for every rank."""
    return [(get(r), ref[r["l2g"][level][: r["owned"][level]]]) for r in res]


@pytest.mark.parametrize("dims,n,orders", SWEEP_CASES,
                         ids=[f"dims{i}-n{i}" for i in range(len(SWEEP_CASES))])
def test_shape_sweep_as_threads(pm, dims, n, orders):
    import scipy.sparse.linalg as spla

    from oracle import pmg_oracle as po

    t_start = time.perf_counter()
    world, L = int(np.prod(dims)), len(orders)
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=K, warp=warp)
    rng = np.random.default_rng(11)
    inputs = {"u": [rng.standard_normal(A.ndofs) for A in ops],
              "w": [rng.integers(-40, 41, A.ndofs).astype(np.float64) for A in ops]}
    if orders[0] == 1:
        g = np.random.default_rng(5).standard_normal(ops[0].ndofs)
        g[mesh.boundary_marker(1).astype(bool)] = 0.0
        inputs["g"] = g
    res = _run_as_threads(pm, n, dims, orders, inputs)
    t_gpu = time.perf_counter()

    # the premises: the ranks are the ones of the host table, and every global dof has one owner
    no_interior = PREMISES[(dims, n)][0]
    for i, P in enumerate(orders):
        facts = rank_facts(dims, n, P)
        assert [r["cell_lists"][i] for r in res] == [(f[5], f[6]) for f in facts]
        assert [r for r in range(world) if res[r]["cell_lists"][i][0] == 0] == no_interior
        owners = np.concatenate([r["l2g"][i][: r["owned"][i]] for r in res])
        assert np.array_equal(np.sort(owners), np.arange(ops[i].ndofs))
    worst = {}
    for i, (P, A) in enumerate(zip(orders, ops)):
        ug, wg = inputs["u"][i], inputs["w"][i]
        # operator: stale ghosts on input, current ones afterwards
        ref = A.apply(ug)
        worst[f"apply P{P}"] = e = _maxrel(_owned(res, lambda r: r["apply"][i], i, ref), ref)
        assert e < 1e-12, (P, e)
        for r in res:
            assert np.array_equal(r["input_after"][i], ug[r["l2g"][i]]), P
        # reverse scatter, exact: every ghost copy lands in its owner, one-way neighbours included
        want = wg.copy()
        for rank, r in enumerate(res):
            gh = r["l2g"][i][r["owned"][i]:]
            np.add.at(want, gh, _ghost_value(gh, rank))
        for a, w in _owned(res, lambda r: r["rev"][i], i, want):
            assert np.array_equal(a, w), P
        assert not np.array_equal(want, wg)
        # reductions
        for r in res:
            assert abs(r["dot"][i] - ug @ ug) < 1e-10 * (ug @ ug)
            assert r["linf"][i] == np.abs(ug).max()
        ref = A.diag_inverse()
        worst[f"dinv P{P}"] = e = _maxrel(_owned(res, lambda r: r["dinv"][i], i, ref), ref)
        assert e < 1e-12, (P, e)
    for i in range(L - 1):
        ref = it[i].interpolate(inputs["u"][i])
        worst[f"prolong {orders[i]}->{orders[i + 1]}"] = e = _maxrel(_owned(res, lambda r: r["prolong"][i], i + 1, ref), ref)
        assert e < 1e-13, (orders[i], e)
        ref = it[i].reverse_interpolate(inputs["u"][i + 1])
        worst[f"restrict {orders[i + 1]}->{orders[i]}"] = e = _maxrel(_owned(res, lambda r: r["restrict"][i], i, ref), ref)
        assert e < 1e-12, (orders[i], e)

    # smoother bounds, then the cycles with the library's bounds in the oracle's smoothers
    assert all(r["eig"] == res[0]["eig"] for r in res)
    for got, ref in zip(res[0]["eig"], eigs):
        assert abs(got[1] - ref[1]) < 1e-8 * ref[1], (got, ref)
    for s, e in zip(sm, res[0]["eig"]):
        s.eig_range = e
    xo = np.zeros_like(b)
    for c in range(2):
        xo = mg.apply(b, xo, compute_rnorm=True)
        worst[f"cycle {c}"] = e = _maxrel(_owned(res, lambda r: r["cycles"][c], -1, xo), xo)
        assert e < 1e-10, (c, e)
        for r in res:
            assert abs(r["rnorms"][c] - mg.rnorm) < 1e-8 * mg.rnorm, (c, r["rnorms"][c], mg.rnorm)
    expect = (2 * K + 1) + 2 * K * (L - 2) + (K - 1) + 2 * (L - 1) - (L - 1)
    assert [r["exchanges"] for r in res] == [expect] * world

    ocg = po.CGSolver()
    ocg.set_max_iterations(30)
    ocg.set_tolerance(1e-9)
    xr = np.zeros_like(b)
    its_ref = ocg.solve(ops[-1], xr, b, precond=lambda r_: mg.apply(r_, np.zeros_like(r_)))
    assert [r["pcg_its"] for r in res] == [its_ref] * world
    worst["pcg"] = e = _maxrel(_owned(res, lambda r: r["pcg"], -1, xr), xr)
    assert e < 1e-8, e

    if orders[0] == 1:
        xs = spla.spsolve(ops[0].assemble_csr().tocsc(), inputs["g"])
        for name in ("rep", "rep_full", "dis"):
            worst[name] = e = _maxrel(_owned(res, lambda r: r[name], 0, xs), xs)
            assert e < 1e-7, (name, e)
            assert all(r[name + "_its"] == res[0][name + "_its"] for r in res), name
            assert all(r[name + "_levels"][1:] == res[0][name + "_levels"][1:] for r in res), name
        assert all(r["rep_levels"] == res[0]["rep_levels"] for r in res)  # the gathered matrix: level 0 as well
        lu = spla.splu(ops[0].assemble_csr().tocsc())

        def exact(u0, b0):
            u0[:] = lu.solve(b0)

        mgo = po.MultigridPreconditioner(ops, sm, it, mesh.boundary_marker(1), coarse_solver=exact)
        xo = np.zeros_like(b)
        for c in range(2):
            xo = mgo.apply(b, xo)
            worst[f"amg cycle {c}"] = e = _maxrel(_owned(res, lambda r: r["amg_cycles"][c], -1, xo), xo)
            assert e < 1e-7, (c, e)
    print(f"\n{dims} on {n}, degrees {orders}: {t_gpu - t_start:.2f} s oracle set-up + ranks, "
          f"{time.perf_counter() - t_gpu:.2f} s comparison; worst " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- part B: the same chains through the halo windows, ranks as processes -----------------------------------------
_ROUTES = {WINDOW_CASES[0][:2]: ("windows", "window-comm", "windows-split"), WINDOW_CASES[1][:2]: ("windows",)}
_PROCESS_CASES = [pytest.param(d, n, o, r, id=f"dims{i}-n{i}-{r}")
                  for i, (d, n, o) in enumerate(WINDOW_CASES) for r in _ROUTES[(d, n)]]


@pytest.mark.parametrize("dims,n,orders,route", _PROCESS_CASES)
def test_mixed_forms_through_halo_windows(dims, n, orders, route, built):
    """Rank 0 has an interior and a boundary cell list, both merged: on route "windows" and "window-comm" it takes its
    exchange whole, in one launch in front of one launch over all patches.  The other ranks have no interior list and
    run put / (nothing) / get / boundary.  "windows-split" is the control: every rank split."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = int(np.prod(dims))
    t0 = time.perf_counter()
    res = _run_ranks(_worker, world, (n, dims, orders, route))
    # the ranks differ as the host table says: one merged launch per cell list that is not empty
    for i, P in enumerate(orders):
        facts = rank_facts(dims, n, P)
        assert [out["cell_lists"][i] for out in res] == [(f[5], f[6]) for f in facts]
        assert [out["launches"][i] for out in res] == [2 if f[5] else 1 for f in facts]
        assert [out["neighbors"][i] for out in res] == [f[3] for f in facts]
        assert [out["ghosts"][i] for out in res] == [f[2] for f in facts]
    assert res[0]["cell_lists"][-1][0] > 0 and [r for r, out in enumerate(res) if out["cell_lists"][-1][0] == 0] == \
        PREMISES[(dims, n)][0]
    # _assert_rank_results of tests/test_gpu_distributed.py without its coarsening ratios (levels of 100 dofs)
    for out in res:
        assert all(g > 0 for g in out["ghosts"])
        assert max(out["apply_err"]) < 1e-12, out["apply_err"]
        for got, ref in zip(out["eig"], out["eig_ref"]):
            assert abs(got[1] - ref[1]) < 1e-8 * ref[1]
        for e, rn in out["vcycle_err"]:
            assert e < 1e-10 and rn < 1e-8
        assert out["exchanges_per_cycle"][0] == out["exchanges_per_cycle"][1], out["exchanges_per_cycle"]
        assert max(out["amg_vcycle_err"]) < 1e-7, out["amg_vcycle_err"]
        assert out["rep_err"] < 1e-7 and max(out["rep_vcycle_err"]) < 1e-5, (out["rep_err"], out["rep_vcycle_err"])
    assert all(out["rep_its"] == res[0]["rep_its"] and out["rep_levels"] == res[0]["rep_levels"] for out in res)
    assert res[0]["rep_its"] <= 14
    for out in res:
        assert abs(out["rep_full_its"] - out["rep_its"]) <= 1 and out["rep_dist_vs_full"] < 1e-7, (
            out["rep_full_its"], out["rep_its"], out["rep_dist_vs_full"])
        assert out["dis_its"] <= 14 and out["dis_err"] < 1e-7, (out["dis_its"], out["rep_its"], out["dis_err"])
    assert all(out["dis_levels"][1:] == res[0]["dis_levels"][1:] for out in res)
    # eight cycles eager, the same eight replayed as a hipGraph
    for out in res:
        assert out["graph_replays"] >= 7 and out["graph_vs_eager"] < 1e-12, (out["graph_replays"], out["graph_vs_eager"])
        if route == "window-comm":
            assert out["long_allreduce_ok"] and out["long_allgather_ok"]
    print(f"\n{dims} on {n}, degrees {orders}, route {route}: {time.perf_counter() - t0:.2f} s")
