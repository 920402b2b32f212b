"""The distributed AMG set-up (pmg_amg_create_distributed: the first coarsening per rank, only level 1 gathered) pinned
to the restated set-up of oracle/amg_oracle.py through the rank-wise export: every rank's rows of A_0 and of P_0, the
gathered A_1 = P_0^T A_0 P_0, the global numbering of the aggregates, and the bound rho_0 of the partitioned operator.
The ranks are host threads of this process (the thread world of tests/test_gpu_distributed.py)."""
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_distributed import _ThreadComm, _ThreadWorld, warp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _distributed_setup(pm, n, dims):
    """Every rank's exports of the distributed set-up: a list of dicts, one per rank."""
    world = int(np.prod(dims))
    W = _ThreadWorld(world)
    res, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                part = pm.BoxPartition(n, dims, rank, warp=warp)
                lv = part.level(1)
                layout = pm.make_layout(lv, comm=_ThreadComm(W, rank) if world > 1 else None)
                op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                         lv.bc_marker, layout)
                amg = pm.AmgSolver(op, max_iter=60, rtol=1e-9, global_index=lv.local_to_global,
                                   n_global=part.global_ndofs(1), setup="distributed")
                L = amg.num_levels()
                res[rank] = {"l2g": np.array(lv.local_to_global), "owned": lv.size_local, "info": amg.info(),
                             "A": [amg.export(l, "A") for l in range(L)], "P": [amg.export(l, "P") for l in range(L - 1)]}
                del amg
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
    assert not errors, "\n".join(f"rank {r}:\n{tb}" for r, tb in errors)
    assert all(r is not None for r in res)
    return res


@pytest.mark.parametrize("n,dims", [((8, 8, 16), (1, 1, 2)), ((12, 12, 12), (2, 2, 2))])
def test_distributed_setup_equals_the_restatement(pm, n, dims):
    from oracle import amg_oracle as ao
    from oracle import pmg_oracle as po

    gm = po.BoxMesh(n, warp=warp)
    bc = gm.boundary_marker(1).astype(bool)
    A_ref = po.Laplacian(1, 2.0, gm.dofmap(1), gm.xgeom, gm.geom_dofmap, bc).assemble_csr()
    N = A_ref.shape[0]
    res = _distributed_setup(pm, n, dims)
    assert sorted(np.concatenate([r["l2g"][: r["owned"]] for r in res]).tolist()) == list(range(N))  # a partition

    # rank rows of A_0 (local columns, ghosts included) are the oracle's rows under local_to_global
    rows, cols, vals = [], [], []
    for r in res:
        A0, l2g, no = r["A"][0].tocoo(), r["l2g"], r["owned"]
        assert r["A"][0].shape == (no, l2g.size) and r["info"][0]["rows"] == no
        rows.append(l2g[A0.row]), cols.append(l2g[A0.col]), vals.append(A0.data)
    A_lib = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    assert abs(A_lib - A_ref).max() < 1e-12 * abs(A_ref).max()

    # the global P_0 from the ranks' owned rows (the columns are global aggregate numbers already)
    n1 = res[0]["P"][0].shape[1]
    assert all(r["P"][0].shape == (r["owned"], n1) for r in res)
    rows, cols, vals = [], [], []
    for r in res:
        P = r["P"][0].tocoo()
        rows.append(r["l2g"][P.row]), cols.append(P.col), vals.append(P.data)
    P_lib = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, n1))

    # the restatement: aggregates of each rank's owned block (ghost columns dropped, theta = 0.08), numbered by the
    # order of their smallest global member, smoothed with the full global A_0 and the level's rho_0
    rho0 = res[0]["info"][0]["lambda_max"]
    assert all(r["info"][0]["lambda_max"] == rho0 for r in res)
    agg_g = np.full(N, -1, dtype=np.int64)
    smallest, pass3 = [], 0
    for r in res:
        no, l2g = r["owned"], r["l2g"]
        st = {}
        agg, na = ao.aggregate(r["A"][0][:, :no].tocsr(), 0.08, st)
        pass3 += st["pass3_roots"]
        first = np.full(na, N, dtype=np.int64)
        np.minimum.at(first, agg[agg >= 0], l2g[:no][agg >= 0])
        agg_g[l2g[:no][agg >= 0]] = first[agg[agg >= 0]]  # for now: the aggregate's smallest global member
        smallest.extend(first.tolist())
    assert len(set(smallest)) == len(smallest) == n1
    number = {g: c for c, g in enumerate(sorted(smallest))}
    inside = agg_g >= 0
    agg_g[inside] = [number[g] for g in agg_g[inside].tolist()]
    assert np.array_equal(inside, ~bc)
    print(f"{n} on {dims}: {n1} aggregates, pass-3 roots {pass3}, rho_0 = {rho0:.6f}")
    P_ref = ao.smoothed_prolongator(A_lib, agg_g, n1, rho0)
    assert abs(P_lib - P_ref).max() <= 1e-13 * abs(P_ref).max()

    # A_1: the same bytes on every rank, and the Galerkin product -- the overlap rows and the keyed gather
    A1 = res[0]["A"][1]
    for r in res[1:]:
        B = r["A"][1]
        assert np.array_equal(B.indptr, A1.indptr) and np.array_equal(B.indices, A1.indices)
        assert np.array_equal(B.data, A1.data)
        assert r["info"][1:] == res[0]["info"][1:]
    G = (P_lib.T @ A_lib @ P_lib).tocsr()
    assert abs(A1 - G).max() < 1e-12 * abs(G).max()

    # rho_0: the power method on the partitioned operator, started from the hash of the global dof numbers
    want = 1.05 * ao.power_bound(A_ref, x0=ao.hashed_start(np.arange(N)))
    assert abs(rho0 - want) < 1e-10 * want
    # ... the same from the distributed set-up run on one rank
    one = _distributed_setup(pm, n, (1, 1, 1))[0]
    assert np.array_equal(one["l2g"], np.arange(N))
    assert abs(one["info"][0]["lambda_max"] - rho0) < 1e-12 * rho0

    # the levels below level 0: the restated build from A_1, its first threshold half of level 0's
    As, Ps, rhos, _ = ao.build(A1, theta0=0.04)
    L = len(res[0]["info"])
    assert [A.shape[0] for A in As] == [i["rows"] for i in res[0]["info"][1:]] and len(As) == L - 1
    for l in range(1, L):
        assert abs(res[0]["info"][l]["lambda_max"] - rhos[l - 1]) < 1e-10 * rhos[l - 1]
        assert abs(res[0]["A"][l] - As[l - 1]).max() < 1e-12 * abs(As[l - 1]).max()
        if l < L - 1:
            assert abs(res[0]["P"][l] - Ps[l - 1]).max() < 1e-12 * abs(Ps[l - 1]).max()
