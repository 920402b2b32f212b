"""The premises of tests/test_gpu_partition_shapes.py, on the host: what `BoxPartition` makes of thin, uneven and
one-cell bricks.  Which ranks have no interior cell list, which exchange with a neighbour in one direction only, which
own no free degree-1 dof, and how large the bricks of the uneven cuts are.  A change of the partitioner that removes
one of these edges fails here; the GPU tests would otherwise quietly turn into repeats of the equal-brick ones.

Per rank: (owned dofs, owned free dofs, ghosts, neighbours, neighbours with traffic in one direction only,
interior cells, boundary cells)."""
import numpy as np
import pytest

from pmg_dolfinx_amd.mesh import BoxPartition, split_bounds

# (dims, n, orders) of the GPU tests: the thread sweep (part A) and the window cases (part B)
SWEEP_CASES = [((1, 1, 4), (3, 4, 4), (1, 2, 4)),
               ((4, 1, 1), (4, 3, 4), (1, 2, 4)),
               ((1, 3, 1), (3, 5, 4), (1, 2, 4)),
               ((1, 1, 3), (3, 3, 4), (1, 3, 6)),
               ((2, 3, 1), (3, 4, 4), (1, 2)),
               ((2, 2, 2), (2, 2, 2), (2, 4))]
WINDOW_CASES = [((1, 1, 3), (3, 4, 3), (1, 2, 4)),
                ((1, 1, 4), (3, 4, 4), (1, 2))]

_THIN4 = [(40, 6, 20, 2, 1, 12, 12), (20, 6, 60, 3, 1, 0, 36), (20, 6, 60, 3, 1, 0, 36), (20, 0, 40, 2, 1, 0, 24)]
TABLE = {
    ((1, 1, 3), (3, 4, 3), 1): [(40, 6, 20, 2, 1, 12, 12), (20, 6, 60, 2, 0, 0, 36), (20, 0, 40, 2, 1, 0, 24)],
    ((1, 1, 3), (3, 4, 3), 4): [(1105, 660, 884, 2, 1, 12, 12), (884, 660, 1989, 2, 0, 0, 36),
                                (884, 495, 1105, 2, 1, 0, 24)],
    ((1, 1, 4), (3, 4, 4), 1): _THIN4,
    ((4, 1, 1), (4, 3, 4), 1): _THIN4,  # the cut along x, the slowest axis
    ((1, 3, 1), (3, 5, 4), 2): [(189, 70, 126, 1, 0, 12, 12), (252, 140, 315, 2, 0, 12, 36),
                                (252, 105, 189, 1, 0, 12, 24)],
    ((1, 1, 3), (3, 3, 4), 6): [(2527, 1734, 2166, 2, 1, 9, 9), (2166, 1734, 4693, 2, 0, 0, 27),
                                (4332, 3179, 2527, 2, 1, 9, 18)],
}


def rank_facts(dims, n, P):
    out = []
    for r in range(int(np.prod(dims))):
        lv = BoxPartition(n, dims, r).level(P)
        free = int((lv.bc_marker[: lv.size_local] == 0).sum())
        one_way = sum((s == 0) != (c == 0) for s, c in zip(lv.send_counts, lv.recv_counts))
        out.append((lv.size_local, free, lv.num_ghosts, len(lv.neighbors), one_way, len(lv.lcells), len(lv.bcells)))
    return out


@pytest.mark.parametrize("key", sorted(TABLE), ids=lambda k: f"dims{k[0]}-n{k[1]}-P{k[2]}".replace(" ", ""))
def test_rank_table(key):
    dims, n, P = key
    assert rank_facts(dims, n, P) == TABLE[key]


def test_six_ranks_uneven_in_both_cut_directions():
    facts = rank_facts((2, 3, 1), (3, 4, 4), 2)
    assert len(facts) == 6 and all(f[3] == 5 for f in facts)              # faces and edges: everybody but itself
    assert [r for r, f in enumerate(facts) if f[5] == 0] == [1, 4]        # the one-cell bricks in y, not the lowest
    assert sorted(f[4] for f in facts) == [0, 0, 2, 2, 2, 2]
    assert split_bounds(3, 2) == [0, 1, 3] and split_bounds(4, 3) == [0, 1, 2, 4]
    p1 = rank_facts((2, 3, 1), (3, 4, 4), 1)
    assert all(f[1] > 0 for f in p1)                                      # every rank owns a free degree-1 dof here


def test_one_cell_per_rank():
    for P in (2, 4):
        facts = rank_facts((2, 2, 2), (2, 2, 2), P)
        assert all(f[3] == 7 and f[5] + f[6] == 8 for f in facts)         # every rank holds all eight cells
        assert [f[5] for f in facts] == [1, 0, 0, 0, 0, 0, 0, 0]          # the lowest rank owns all its cell's dofs
    facts = rank_facts((2, 2, 2), (2, 2, 2), 2)
    assert facts[7][:2] == (8, 1)
    assert BoxPartition((2, 2, 2)).level(1).bc_marker.sum() == 26         # degree 1: a single free dof, no such level


def test_brick_sizes_of_the_uneven_cuts():
    assert np.diff(split_bounds(4, 3)).tolist() == [1, 1, 2]              # (1,1,3) on (3,3,4)
    assert np.diff(split_bounds(5, 3)).tolist() == [1, 2, 2]              # (1,3,1) on (3,5,4)
    assert np.diff(split_bounds(4, 4)).tolist() == [1, 1, 1, 1]
    assert np.diff(split_bounds(3, 3)).tolist() == [1, 1, 1]
    for dims, n, _ in SWEEP_CASES + WINDOW_CASES:
        cells = [BoxPartition(n, dims, r).ncells_owned for r in range(int(np.prod(dims)))]
        assert sum(cells) == int(np.prod(n)) and min(cells) > 0


# per case, the same on every level: ranks with an empty interior list, ranks with a one-way neighbour, ranks that own
# no free degree-1 dof (None: the case has no degree-1 level)
PREMISES = {
    ((1, 1, 4), (3, 4, 4)): ([1, 2, 3], [0, 1, 2, 3], [3]),
    ((4, 1, 1), (4, 3, 4)): ([1, 2, 3], [0, 1, 2, 3], [3]),
    ((1, 3, 1), (3, 5, 4)): ([], [], []),  # two cell layers in the upper bricks: uneven, nothing else
    ((1, 1, 3), (3, 3, 4)): ([1], [0, 2], []),
    ((2, 3, 1), (3, 4, 4)): ([1, 4], [0, 2, 3, 5], []),
    ((2, 2, 2), (2, 2, 2)): ([1, 2, 3, 4, 5, 6, 7], [], None),
    ((1, 1, 3), (3, 4, 3)): ([1, 2], [0, 2], [2]),
}


@pytest.mark.parametrize("dims,n,orders", SWEEP_CASES + WINDOW_CASES)
def test_premises_of_the_gpu_cases(dims, n, orders):
    no_interior, one_way, no_free = PREMISES[(dims, n)]
    for P in orders:
        facts = rank_facts(dims, n, P)
        assert [r for r, f in enumerate(facts) if f[5] == 0] == no_interior, (P, facts)
        assert [r for r, f in enumerate(facts) if f[4] > 0] == one_way, (P, facts)
        assert all(f[6] > 0 for f in facts)
        # a rank with both lists next to one without: the pair that can take different forms of an application
        if no_interior:
            assert any(f[5] > 0 and f[6] > 0 for f in facts)
    assert (orders[0] == 1) == (no_free is not None)
    if no_free is not None:
        assert [r for r, f in enumerate(rank_facts(dims, n, 1)) if f[1] == 0] == no_free


@pytest.mark.parametrize("dims,n,orders", SWEEP_CASES + WINDOW_CASES)
def test_both_sides_of_every_halo_plan_agree(dims, n, orders):
    """What the thread transport of the GPU tests asserts at run time, zero counts included: a rank lists a neighbour
    exactly when that neighbour lists it, and what one side sends the other receives, entry by entry."""
    world = int(np.prod(dims))
    parts = [BoxPartition(n, dims, r) for r in range(world)]
    for P in orders:
        lvs = [p.level(P) for p in parts]
        owned = np.concatenate([lv.local_to_global[: lv.size_local] for lv in lvs])
        assert np.array_equal(np.sort(owned), np.arange(parts[0].global_ndofs(P)))
        zero_segments = 0
        for r, lv in enumerate(lvs):
            assert lv.neighbors == sorted(set(lv.neighbors)) and r not in lv.neighbors
            assert len(lv.send_counts) == len(lv.recv_counts) == len(lv.neighbors)
            assert sum(lv.recv_counts) == lv.num_ghosts and sum(lv.send_counts) == len(lv.send_indices)
            off = 0
            for i, q in enumerate(lv.neighbors):
                lq = lvs[q]
                assert r in lq.neighbors, (P, r, q)
                j = lq.neighbors.index(r)
                assert lq.send_counts[j] == lv.recv_counts[i] and lq.recv_counts[j] == lv.send_counts[i], (P, r, q)
                assert lv.send_counts[i] + lv.recv_counts[i] > 0
                zero_segments += (lv.send_counts[i] == 0) + (lv.recv_counts[i] == 0)
                cnt, so = lv.recv_counts[i], sum(lq.send_counts[:j])
                sent = lq.local_to_global[lq.send_indices[so: so + cnt]]
                assert np.array_equal(sent, lv.local_to_global[lv.size_local + off: lv.size_local + off + cnt])
                off += cnt
        # a zero-length segment has its counterpart on the other rank
        assert zero_segments % 2 == 0
