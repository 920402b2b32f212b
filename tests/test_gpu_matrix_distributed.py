"""The distributed assembled operator (``pmg_matrix_create_distributed``, ``MatrixOperator(op, distributed=True)``):
ghost columns, the diag / off-diag split of src/csr.hpp:114-126 and the two-phase product of :252-270, on the
partitions of tests/test_partition_shapes.py.

Part A: the ranks as threads of this process (``rank_harness._ThreadWorld``: exchange and all-reduce through the
callbacks of the C ABI).  Nothing is judged inside a rank; every rank's results are compared afterwards with the
single-domain oracle -- ``po.Laplacian(...).assemble_csr()`` and ``po.build_hierarchy`` -- the truth for a rank's matrix
being the rows ``l2g[:size_local]`` and the columns ``l2g`` of the oracle's.
Part B: the thin chain with the ranks as processes that exchange through halo windows, the assembled cycle eager and
replayed as a hipGraph, once with the merged plan (the exchange taken whole in front of one full-row launch) and once
with every level split.

Tolerances are DESIGN.md section 2's: 1e-12 relative for a product, a diagonal or a matrix entry, 1e-10 after a
Chebyshev solve or a V-cycle."""
import os
import threading
import time

import numpy as np
import pytest

from rank_harness import _reporting, _run_ranks, _ThreadComm, _ThreadWorld
from test_gpu_distributed import warp
from test_matrix_pattern_host import CASES, global_pattern, restricted_pattern

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 3                 # Chebyshev iterations per smooth
BARRIER_SECONDS = 60  # the meshes are tiny: a rank that returned early fails the test quickly
CG_ITS, CG_RTOL = 15, 1e-6  # the run of tests/test_gpu_matrix_operator.py's comparison of the two operators under CG
LEVEL_SETS = ("coarsest", "all")


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _stale(lv, ug):
    """The rank's part of the global vector `ug` with its ghost entries not yet received."""
    xl = np.zeros(lv.ndofs)
    xl[: lv.size_local] = ug[lv.local_to_global[: lv.size_local]]
    return xl


def _vector(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _one_eager_cycle(H, xv):
    """Forward scatters of one eager cycle, over all levels (a replayed cycle issues its scatters once, at capture)."""
    H.mg.set_graph(False)
    before = sum(l.forward_scatters() for l in H.layouts)
    H.mg.apply(H.rhs[-1], xv)
    H.mg.set_graph(None)
    return sum(l.forward_scatters() for l in H.layouts) - before


def _rank_body(pm, rank, world, n, dims, orders, comm, inputs):
    """What one rank computes on the device; nothing is judged here (a rank that failed a check of its own would
    leave the others waiting in the next collective)."""
    H = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=K, proc_dims=dims, rank=rank, size=world, warp=warp,
                            comm=comm)
    L = len(orders)
    out = {"eig": H.eig_ranges, "l2g": [np.array(lv.local_to_global) for lv in H.levels],
           "owned": [lv.size_local for lv in H.levels], "bc": [np.array(lv.bc_marker) for lv in H.levels],
           "csr": [], "split": [], "shape": [], "norm": [], "dinv": [], "same_bits": [], "product": [],
           "input_after": [], "current": [], "free": [], "cheb": [], "cg": [], "cg_free": []}
    mats = []
    for i, (lv, layout, op) in enumerate(zip(H.levels, H.layouts, H.operators)):
        nl = lv.size_local
        M = pm.MatrixOperator(op, distributed=True)
        mats.append(M)
        rp, ci, v = M.export()
        out["csr"].append((rp.copy(), ci.copy(), v.copy()))
        out["split"].append(tuple(a.copy() for a in M.export_split()))
        out["shape"].append((M.rows, M.cols, M.nnz))
        out["norm"].append(M.norm())  # collective
        d = pm.Vector(layout)
        M.get_diag_inverse(d)
        out["dinv"].append(d.data_copy()[:nl].copy())
        M.update_values()
        rp2, ci2, v2 = M.export()
        out["same_bits"].append(rp2.tobytes() == rp.tobytes() and ci2.tobytes() == ci.tobytes()
                                and v2.tobytes() == v.tobytes())
        # the product: stale ghosts in, 9 in the output
        x, y = _vector(pm, layout, _stale(lv, inputs["u"][i])), pm.Vector(layout)
        y.set(9.0)
        M(x, y)
        out["product"].append(y.data_copy().copy())
        out["input_after"].append(x.data_copy().copy())
        # ... and with the ghosts now current: no exchange, one launch over whole rows
        y1 = pm.Vector(layout)
        y1.set(9.0)
        before = layout.forward_scatters()
        M.apply_ghosts_current(x, y1)
        out["current"].append((y1.data_copy().copy(), layout.forward_scatters() - before))
        x2, z = _vector(pm, layout, _stale(lv, inputs["u"][i])), pm.Vector(layout)
        op(x2, z)
        out["free"].append(z.data_copy()[:nl].copy())
        # Chebyshev(3) from a non-zero guess
        xc, bc_ = _vector(pm, layout, _stale(lv, inputs["u"][i])), _vector(pm, layout, _stale(lv, inputs["b"][i]))
        H.smoothers[i].solve(M, xc, bc_)
        out["cheb"].append(xc.data_copy()[:nl].copy())
        # Jacobi-CG on the matrix and on the matrix-free operator
        for key, A in (("cg", M), ("cg_free", op)):
            cg = pm.CGSolver(layout)
            cg.set_max_iterations(CG_ITS)
            cg.set_tolerance(CG_RTOL)
            xs = pm.Vector(layout)
            xs.set(0.0)
            its = cg.solve(A, xs, bc_)
            out[key].append((its, xs.data_copy()[:nl].copy()))
            del cg, xs
    # the cycle: the matrix-free hierarchy first, with and without the exchange bookkeeping ...
    nf = H.levels[-1].size_local
    xv = H.new_vector()
    xv.set(0.0)
    H.mg.set_fused_restriction(0)
    H.mg.apply(H.rhs[-1], xv)
    out["exchanges_free"] = _one_eager_cycle(H, xv)
    # ... then with assembled levels
    out["cycles"], out["exchanges"], out["exchanges_no_local"] = {}, {}, {}
    for name in LEVEL_SETS:
        levels = (0,) if name == "coarsest" else tuple(range(L))
        for i in range(L):
            H.mg.set_level_matrix(i, mats[i] if i in levels else None)
        xv.set(0.0)
        out["cycles"][name] = []
        for _ in range(2):
            H.mg.apply(H.rhs[-1], xv)
            out["cycles"][name].append(xv.data_copy()[:nf].copy())
        out["exchanges"][name] = _one_eager_cycle(H, xv)
        # PMG_LOCAL_CORRECTION=0 (read at every cycle): one rank sets it while all of them wait
        comm.W.wait()
        if rank == 0:
            os.environ["PMG_LOCAL_CORRECTION"] = "0"
        comm.W.wait()
        try:
            out["exchanges_no_local"][name] = _one_eager_cycle(H, xv)
        finally:
            comm.W.wait()
            if rank == 0:
                del os.environ["PMG_LOCAL_CORRECTION"]
            comm.W.wait()
    for i in range(L):
        H.mg.set_level_matrix(i, None)
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
    os.environ.pop("PMG_LOCAL_CORRECTION", None)
    assert not errors, "\n".join(f"rank {r}:\n{tb}" for r, tb in sorted(errors))
    assert all(r is not None for r in res)
    return res


def _maxrel(parts, ref):
    return max(float(np.abs(a - b).max()) for a, b in parts) / max(float(np.abs(ref).max()), 1e-300)


def _owned(res, get, level, ref):
    """(rank's owned values of level `level`, the oracle's at the same dofs) for every rank."""
    return [(get(r), ref[r["l2g"][level][: r["owned"][level]]]) for r in res]


class _Lv:
    """The two members of a level restricted_pattern reads."""

    def __init__(self, size_local, l2g):
        self.size_local, self.local_to_global = size_local, l2g


@pytest.mark.parametrize("dims,n,orders", CASES, ids=[f"dims{i}" for i in range(len(CASES))])
def test_distributed_matrix_as_threads(pm, dims, n, orders):
    import scipy.sparse as sp

    from oracle import pmg_oracle as po

    t_start = time.perf_counter()
    world, L = int(np.prod(dims)), len(orders)
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=K, warp=warp)
    rng = np.random.default_rng(23)
    inputs = {"u": [rng.standard_normal(A.ndofs) for A in ops], "b": [rng.standard_normal(A.ndofs) for A in ops]}
    res = _run_as_threads(pm, n, dims, orders, inputs)
    t_gpu = time.perf_counter()
    worst = {}
    for i, (P, A) in enumerate(zip(orders, ops)):
        owners = np.concatenate([r["l2g"][i][: r["owned"][i]] for r in res])
        assert np.array_equal(np.sort(owners), np.arange(A.ndofs))  # every global row on exactly one rank
        ref = A.assemble_csr()
        amax = float(np.abs(ref.data).max())
        fro = float(np.sqrt((ref.data ** 2).sum()))
        G = global_pattern(n, P)
        ug, bg = inputs["u"][i], inputs["b"][i]
        for rank, r in enumerate(res):
            nl, l2g = r["owned"][i], r["l2g"][i]
            rp, ci, v = r["csr"][i]
            od, brows = r["split"][i]
            assert r["shape"][i] == (nl, l2g.size, ci.size)
            # the pattern: the oracle's, restricted and renumbered; the split; the boundary rows
            wrp, wci = restricted_pattern(G, _Lv(nl, l2g))
            assert np.array_equal(rp, wrp) and np.array_equal(ci, wci), (P, rank)
            first_ghost = np.array([rp[k] + np.searchsorted(ci[rp[k]: rp[k + 1]], nl) for k in range(nl)],
                                   dtype=np.int32)
            assert np.array_equal(od, first_ghost), (P, rank)
            assert np.array_equal(brows, np.flatnonzero(first_ghost < rp[1:]).astype(np.int32)), (P, rank)
            # the values
            got = sp.csr_matrix((v, ci, rp), shape=(nl, l2g.size))
            want = ref[l2g[:nl]][:, l2g]
            diff = abs(got - want)
            worst[f"values P{P}"] = e = max(worst.get(f"values P{P}", 0.0), (diff.max() if diff.nnz else 0.0) / amax)
            assert e <= 1e-12, (P, rank, e)
            assert abs(r["norm"][i] - fro) <= 1e-12 * fro, (P, rank, r["norm"][i], fro)
            assert r["same_bits"][i], (P, rank)
            marked = r["bc"][i][:nl].astype(bool)
            assert np.array_equal(r["dinv"][i][marked], np.ones(int(marked.sum()))), (P, rank)
            # the product: the ghosts of the input current, the ghosts of the output untouched
            assert np.array_equal(r["input_after"][i], ug[l2g]), (P, rank)
            assert np.array_equal(r["product"][i][nl:], np.full(l2g.size - nl, 9.0)), (P, rank)
        ref_d = A.diag_inverse()
        worst[f"dinv P{P}"] = e = _maxrel(_owned(res, lambda r: r["dinv"][i], i, ref_d), ref_d)
        assert e < 1e-12, (P, e)
        ref_y = A.apply(ug)
        worst[f"product P{P}"] = e = _maxrel(_owned(res, lambda r: r["product"][i][: r["owned"][i]], i, ref_y), ref_y)
        assert e < 1e-12, (P, e)
        worst[f"one launch P{P}"] = e = _maxrel(_owned(res, lambda r: r["current"][i][0][: r["owned"][i]], i, ref_y),
                                                ref_y)
        assert e < 1e-12, (P, e)
        for r in res:
            y1, scatters = r["current"][i]
            assert scatters == 0 and np.array_equal(y1[r["owned"][i]:], r["product"][i][r["owned"][i]:]), P
        worst[f"vs matrix-free P{P}"] = e = _maxrel([(r["product"][i][: r["owned"][i]], r["free"][i]) for r in res],
                                                    ref_y)
        assert e < 1e-12, (P, e)
        # Chebyshev(3) from a non-zero guess, the library's bounds in the oracle's smoother
        assert all(r["eig"] == res[0]["eig"] for r in res)
        xc = po.Chebyshev(res[0]["eig"][i], K).solve(A, ug.copy(), bg)
        worst[f"cheb P{P}"] = e = _maxrel(_owned(res, lambda r: r["cheb"][i], i, xc), xc)
        assert e < 1e-10, (P, e)
        # Jacobi-CG: the iteration count of the matrix-free operator, the same iterate
        its = [r["cg"][i][0] for r in res]
        assert its == [r["cg_free"][i][0] for r in res] and len(set(its)) == 1, (P, its)
        scale = max(float(np.abs(r["cg_free"][i][1]).max()) for r in res)
        worst[f"cg P{P}"] = e = max(float(np.abs(r["cg"][i][1] - r["cg_free"][i][1]).max()) for r in res) / scale
        assert e < 1e-9, (P, e)

    # the cycles, with the library's bounds in the oracle's smoothers
    for s, e in zip(sm, res[0]["eig"]):
        s.eig_range = e
    xo, want = np.zeros_like(b), []
    for c in range(2):
        xo = mg.apply(b, xo)
        want.append(xo.copy())
    for name in LEVEL_SETS:
        for c in range(2):
            worst[f"cycle {c} {name}"] = e = _maxrel(_owned(res, lambda r: r["cycles"][name][c], -1, want[c]), want[c])
            assert e < 1e-10, (name, c, e)
        for r in res:
            # the exchange bookkeeping holds for an assembled level as for a matrix-free one
            assert r["exchanges"][name] == r["exchanges_free"], (name, r["exchanges"][name], r["exchanges_free"])
            assert r["exchanges"][name] < r["exchanges_no_local"][name], (name, r["exchanges_no_local"][name])
    expect = (2 * K + 1) + 2 * K * (L - 2) + (K - 1) + 2 * (L - 1) - (L - 1)
    assert [r["exchanges_free"] for r in res] == [expect] * world
    print(f"\n{dims} on {n}, degrees {orders}: {t_gpu - t_start:.2f} s oracle set-up + ranks, "
          f"{time.perf_counter() - t_gpu:.2f} s comparison; worst "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_same_arrays_on_a_ghost_free_layout(pm):
    """On a single-domain layout the new constructor gives the arrays of the old one, and no boundary row."""
    for nn, P in ((4, 2), (3, 3)):
        part = pm.BoxPartition(nn, warp=warp)
        lv = part.level(P)
        layout = pm.make_layout(lv)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                                 layout)
        old, new = pm.MatrixOperator(op), pm.MatrixOperator(op, distributed=True)
        for a, c in zip(old.export(), new.export()):
            assert a.dtype == c.dtype and a.tobytes() == c.tobytes()
        assert (new.rows, new.cols, new.nnz) == (old.rows, old.cols, old.nnz) == (lv.ndofs, lv.ndofs, old.nnz)
        od, brows = new.export_split()
        rp = new.export()[0]
        assert brows.size == 0 and np.array_equal(od, rp[1:])
        for a, c in zip(old.export_split(), (od, brows)):
            assert np.array_equal(a, c)
        u = np.random.default_rng(P).standard_normal(lv.ndofs)
        x, y0, y1 = _vector(pm, layout, u), pm.Vector(layout), pm.Vector(layout)
        before = layout.forward_scatters()
        old(x, y0)
        new(x, y1)
        assert layout.forward_scatters() == before  # no halo: no exchange, one launch
        assert y0.data_copy().tobytes() == y1.data_copy().tobytes()
        assert old.norm() == new.norm()


# ---- part B: the window route, ranks as processes ------------------------------------------------------------------
WINDOW_CASE = ((1, 1, 4), (3, 4, 4), (1, 2))


def _window_worker_body(rank, world, port, n, dims, orders, route):
    import torch
    import torch.distributed as dist

    from oracle import pmg_oracle as po

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("PMG_WINDOW_TIMEOUT_MS", "20000")  # the ranks time-slice one GPU: generous, still bounded
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm

        torch.cuda.set_device(0)
        if route == "split":  # no merged plan: no level takes its exchange whole, the split form meets the window flags
            pm.set_merge_threshold(0)
        comm = pm.TorchComm(halo="windows")  # halo windows, reductions on the gloo callbacks
        H = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=K, proc_dims=dims, rank=rank, size=world, warp=warp,
                                comm=comm, assembled_levels=tuple(range(len(orders))))
        lvf = H.levels[-1]
        nf, l2g = lvf.size_local, lvf.local_to_global
        out = {"eig": H.eig_ranges, "launches": [op.launches_per_apply() for op in H.operators],
               "distributed": [H.matrices[i].distributed for i in range(len(orders))],
               "boundary_rows": [int(H.matrices[i].export_split()[1].size) for i in range(len(orders))]}
        # the product on the finest level against the oracle's
        mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=K, warp=warp)
        ug = np.random.default_rng(11).standard_normal(ops[-1].ndofs)
        xl = np.zeros(lvf.ndofs)
        xl[:nf] = ug[l2g[:nf]]
        x, y = pm.Vector(H.layouts[-1]), pm.Vector(H.layouts[-1])
        x.data.copy_(torch.from_numpy(xl))
        H.matrices[len(orders) - 1](x, y)
        ref = ops[-1].apply(ug)
        out["product_err"] = float(np.abs(y.data_copy()[:nf] - ref[l2g[:nf]]).max() / np.abs(ref).max())
        out["ghosts_current"] = bool(np.array_equal(x.data_copy(), ug[l2g]))
        for s, e in zip(sm, H.eig_ranges):
            s.eig_range = e
        xo, want = np.zeros_like(b), []
        for _ in range(2):
            xo = mg.apply(b, xo)
            want.append(xo.copy())

        def cycles(graph):
            H.mg.set_graph(graph)
            xv = H.new_vector()
            xv.set(0.0)
            errs = []
            for c in range(2):
                H.mg.apply(H.rhs[-1], xv)
                torch.cuda.synchronize()
                errs.append(float(np.abs(xv.data_copy()[:nf] - want[c][l2g[:nf]]).max() / np.abs(want[c]).max()))
            return errs, H.mg.graph_replays()

        out["eager_err"], r0 = cycles(False)
        out["graph_err"], r1 = cycles(True)
        H.mg.set_graph(False)
        out["graph_replays"] = r1 - r0
        dist.barrier()  # nobody frees a window a neighbour may still acknowledge into
        return out
    finally:
        dist.destroy_process_group()


def _window_worker(rank, world, port, n, dims, orders, *rest):
    _reporting(_window_worker_body)(rank, world, port, n, dims, orders, *rest)


@pytest.mark.parametrize("route", ["merged", "split"])
def test_assembled_cycle_through_halo_windows(route, built):
    """Four processes on the thin chain, every level assembled.  "merged": the small levels' operators take the
    single-launch form, so the matrix takes its exchange whole in front of one full-row launch.  "split":
    pmg_set_merge_threshold(0), every product is put / diag / get / off-diag on the window flags."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dims, n, orders = WINDOW_CASE
    world = int(np.prod(dims))
    assert world <= 4
    t0 = time.perf_counter()
    res = _run_ranks(_window_worker, world, (n, dims, orders, route), timeout=240)
    for out in res:
        assert all(out["distributed"]) and all(nb > 0 for nb in out["boundary_rows"])
        assert out["product_err"] < 1e-12 and out["ghosts_current"], out["product_err"]
        assert max(out["eager_err"]) < 1e-10, out["eager_err"]
        assert max(out["graph_err"]) < 1e-10, out["graph_err"]
        assert out["graph_replays"] >= 1, out["graph_replays"]
    print(f"\nroute {route}: launches per apply {[out['launches'] for out in res]}, eager {res[0]['eager_err']}, "
          f"graph {res[0]['graph_err']}; {time.perf_counter() - t0:.2f} s")
