"""Cell-local frames on the CPU: the 48 symmetries of the reference cube, the node / facet maps of the mesh helper,
and the oracles' invariance under them.  Re-framing a cell (permuting and reversing its local axes, left-handed frames
included) changes neither the global matrix, the load vector nor the transfer matrices, so the reference for a mesh
with scrambled frames is the same oracle on the frame-free mesh -- other arrays, another order of every cell's sums.
Bound: 1e-13 relative (the proper rotations reach 5e-16 with a signed determinant already; the reflections need
|det J|, see profiles/cell_frames.md)."""
import numpy as np
import pytest

from oracle import pmg_oracle as po

N48 = (4, 3, 4)  # 48 cells: every symmetry exactly once
FRAMES48 = np.random.default_rng(48).permutation(48).reshape(N48)
PAIRS = {2: 1, 4: 2, 6: 3, 8: 4}  # fine -> coarse, the pairs of test_irregular_numbering
BOUND = 1e-13


def twist(x):
    """Genuinely trilinear cells: J (and G) vary inside every cell."""
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def pm(built):
    import pmg_dolfinx_amd as pm

    return pm


@pytest.fixture(scope="module")
def meshes(pm):
    return pm.BoxPartition(N48, warp=twist), pm.BoxPartition(N48, warp=twist, cell_frames=FRAMES48)


def test_symmetries_are_48_distinct_bijections(pm):
    syms = pm.cell_symmetries()
    assert len(syms) == 48
    assert syms[0] == ((0, 1, 2), (0, 0, 0), 1)
    assert sorted(s for _, _, s in syms) == [-1] * 24 + [1] * 24
    for P in (1, 2, 3):
        N = (P + 1) ** 3
        maps = [pm.frame_node_map(P, perm, flips) for perm, flips, _ in syms]
        assert np.array_equal(maps[0], np.arange(N))
        for m in maps:
            assert m.dtype == np.int32 and np.array_equal(np.sort(m), np.arange(N))
        assert len({m.tobytes() for m in maps}) == 48
    fmaps = [pm.frame_facet_map(perm, flips) for perm, flips, _ in syms]
    assert np.array_equal(fmaps[0], np.arange(6))
    for f in fmaps:
        assert np.array_equal(np.sort(f), np.arange(6))
    assert len({f.tobytes() for f in fmaps}) == 48


def test_vertex_map_reproduces_the_symmetry(pm):
    """The unit cube's vertices listed in the new frame: new vertex (i0, i1, i2) sits at coordinate i_m (1 - i_m if
    flipped) along old axis perm[m], and the new frame's edge vectors have determinant ``sign``."""
    I, J, K = np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")
    v = np.stack([I.ravel(), J.ravel(), K.ravel()], axis=1).astype(np.float64)  # vertex i*4 + j*2 + k
    for perm, flips, sign in pm.cell_symmetries():
        new = v[pm.frame_node_map(1, perm, flips)]
        for m in range(3):
            want = 1.0 - v[:, m] if flips[m] else v[:, m]
            assert np.array_equal(new[:, perm[m]], want)
        edges = np.stack([new[4] - new[0], new[2] - new[0], new[1] - new[0]], axis=1)  # columns: dx/dxi'_m
        assert np.linalg.det(edges) == pytest.approx(sign, abs=1e-15)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_facet_map_agrees_with_facet_nodes(pm, P):
    for perm, flips, _ in pm.cell_symmetries():
        nmap, fmap = pm.frame_node_map(P, perm, flips), pm.frame_facet_map(perm, flips)
        for f in range(6):
            assert set(nmap[pm.facet_nodes(P, f)]) == set(pm.facet_nodes(P, int(fmap[f])))


def test_partition_arrays_under_frames(pm, meshes):
    """Rows are the frame-free rows listed through the cell's map; coordinates and exterior facets stay right."""
    p0, p1 = meshes
    syms = pm.cell_symmetries()
    fr = FRAMES48.ravel()  # one rank: local cells are the global cells, lexicographic
    assert np.array_equal(p1.cell_frames, fr)
    assert np.array_equal(p0.xgeom, p1.xgeom)
    for c in range(p0.ncells):
        perm, flips, _ = syms[fr[c]]
        assert np.array_equal(p1.geom_dofmap[c], p0.geom_dofmap[c][pm.frame_node_map(1, perm, flips)])
    for P in (1, 2, 3):
        l0, l1 = p0.level(P), p1.level(P)
        for c in range(p0.ncells):
            perm, flips, _ = syms[fr[c]]
            assert np.array_equal(l1.dofmap[c], l0.dofmap[c][pm.frame_node_map(P, perm, flips)])
        # the partition's own, re-framed arrays give the same physical points
        assert _relerr(p1.dof_coordinates(P), p0.dof_coordinates(P)) < 1e-15
        c0, f0 = p0.exterior_facets()
        c1, f1 = p1.exterior_facets()
        assert c1.dtype == np.int32 and f1.dtype == np.int8 and len(c1) == len(c0)
        x0, x1 = p0.facet_point_coordinates(P, c0, f0), p1.facet_point_coordinates(P, c1, f1)
        key0 = {(int(c), int(f)): x for c, f, x in zip(c0, f0, x0)}
        assert np.array_equal(c1, np.sort(c1)) and len(set(zip(c1.tolist(), f1.tolist()))) == len(c1)
        for c, f, x in zip(c1, f1, x1):
            perm, flips, _ = syms[fr[c]]
            old = key0[(int(c), int(pm.frame_facet_map(perm, flips)[f]))]
            # the same points of the same face, in the new frame's order of them
            a = np.array(sorted(map(tuple, np.round(x, 12))))
            b = np.array(sorted(map(tuple, np.round(old, 12))))
            assert np.abs(a - b).max() < 1e-12


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(7)
    return {P: rng.standard_normal(int(np.prod([n * P + 1 for n in N48]))) for P in (1, 2, 3, 4, 6, 8)}


@pytest.mark.parametrize("P", [1, 2, 3, 4, 6, 8])
def test_oracle_invariance_all_48_frames(pm, meshes, vectors, P):
    """numpy and C oracles on the mesh whose 48 cells carry the 48 symmetries, against the frame-free mesh."""
    from oracle import c_oracle as co

    p0, p1 = meshes
    l0, l1 = p0.level(P), p1.level(P)
    kappa = np.random.default_rng(3).uniform(0.5, 3.0, p0.ncells)
    u = vectors[P]
    A0 = po.Laplacian(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    A1 = po.Laplacian(P, kappa, l1.dofmap, p1.xgeom, p1.geom_dofmap, l1.bc_marker)
    assert (A1.detJ > 0).all()
    worst = {}
    worst["apply"] = _relerr(A1.apply(u), A0.apply(u))
    worst["diag_inverse"] = _relerr(A1.diag_inverse(), A0.diag_inverse())
    coords = p0.dof_coordinates(P)
    worst["rhs"] = _relerr(A1.rhs_manufactured(p1.dof_coordinates(P)), A0.rhs_manufactured(coords))
    M0, M1 = A0.assemble_csr(), A1.assemble_csr()
    worst["csr"] = abs(M1 - M0).max() / abs(M0).max()
    C0 = co.CLevel(P, kappa, l0.dofmap, p0.xgeom, p0.geom_dofmap, l0.bc_marker)
    C1 = co.CLevel(P, kappa, l1.dofmap, p1.xgeom, p1.geom_dofmap, l1.bc_marker)
    worst["c apply"] = _relerr(C1.apply(u), C0.apply(u))
    worst["c diag_inverse"] = _relerr(C1.diag_inverse(), C0.diag_inverse())
    worst["c vs numpy"] = _relerr(C1.apply(u), A0.apply(u))
    if P in PAIRS:
        pc = PAIRS[P]
        lc0, lc1 = p0.level(pc), p1.level(pc)
        uc = vectors[pc]
        I0 = po.Interpolator(pc, P, lc0.dofmap, l0.dofmap, lc0.ndofs, l0.ndofs)
        I1 = po.Interpolator(pc, P, lc1.dofmap, l1.dofmap, lc1.ndofs, l1.ndofs)
        worst["interpolate"] = _relerr(I1.interpolate(uc), I0.interpolate(uc))
        worst["reverse_interpolate"] = _relerr(I1.reverse_interpolate(u), I0.reverse_interpolate(u))
        Cc0 = co.CLevel(pc, kappa, lc0.dofmap, p0.xgeom, p0.geom_dofmap, lc0.bc_marker)
        Cc1 = co.CLevel(pc, kappa, lc1.dofmap, p1.xgeom, p1.geom_dofmap, lc1.bc_marker)
        J0, J1 = co.CInterp(Cc0, C0), co.CInterp(Cc1, C1)
        worst["c interpolate"] = _relerr(J1.interpolate(uc), J0.interpolate(uc))
        worst["c reverse_interpolate"] = _relerr(J1.reverse_interpolate(u), J0.reverse_interpolate(u))
    print(f"cell frames, oracle invariance, P = {P}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < BOUND, (k, v)


def test_halo_plans_do_not_depend_on_frames(pm):
    """Four ranks: numbering, ownership, halo lists, cell lists and markers are those of the frame-free partition; a
    rank's dofmap row is the frame-free row as a set, and a cell has the same frame on every rank that holds it."""
    dims = (1, 2, 2)
    syms = pm.cell_symmetries()
    for r in range(4):
        q0 = pm.BoxPartition(N48, dims, r, warp=twist)
        q1 = pm.BoxPartition(N48, dims, r, warp=twist, cell_frames=FRAMES48)
        assert np.array_equal(q0.cell_coords, q1.cell_coords) and q0.ncells_owned == q1.ncells_owned
        cc = q1.cell_coords
        assert np.array_equal(q1.cell_frames, FRAMES48[cc[:, 0], cc[:, 1], cc[:, 2]])
        assert np.array_equal(np.sort(q1.geom_dofmap, axis=1), np.sort(q0.geom_dofmap, axis=1))
        for P in (1, 2, 4):
            l0, l1 = q0.level(P), q1.level(P)
            for name in ("P", "size_local", "num_ghosts", "neighbors", "send_counts", "recv_counts"):
                assert getattr(l0, name) == getattr(l1, name), name
            for name in ("bc_marker", "local_to_global", "ghost_owners", "send_indices", "recv_indices", "lcells",
                         "bcells"):
                a, b = getattr(l0, name), getattr(l1, name)
                assert a.dtype == b.dtype and np.array_equal(a, b), name
            assert l1.dofmap.dtype == np.int32 and l1.dofmap.flags.c_contiguous
            assert np.array_equal(np.sort(l1.dofmap, axis=1), np.sort(l0.dofmap, axis=1))
            assert not np.array_equal(l1.dofmap, l0.dofmap)
            for c in range(q0.ncells):
                perm, flips, _ = syms[q1.cell_frames[c]]
                assert np.array_equal(l1.dofmap[c], l0.dofmap[c][pm.frame_node_map(P, perm, flips)])
            assert _relerr(q1.dof_coordinates(P), q0.dof_coordinates(P)) < 1e-15


def test_cell_frames_argument_is_checked(pm):
    with pytest.raises(ValueError):
        pm.BoxPartition(N48, cell_frames=np.zeros((4, 3, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        pm.BoxPartition(N48, cell_frames=np.full(N48, 48))
    with pytest.raises(ValueError):
        pm.BoxPartition(N48, cell_frames=np.zeros(N48))  # not an integer array
    ident = pm.BoxPartition(N48, warp=twist, cell_frames=np.zeros(N48, dtype=np.int32))
    plain = pm.BoxPartition(N48, warp=twist)
    assert np.array_equal(ident.geom_dofmap, plain.geom_dofmap)
    assert np.array_equal(ident.level(3).dofmap, plain.level(3).dofmap)
    assert ident.geom_dofmap.dtype == np.int32
