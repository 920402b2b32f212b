"""The multi-block mesh helper (tests/multiblock_mesh.py) and the oracles on its meshes, on the CPU.

The helper is the reference geometry of tests/test_gpu_multiblock.py, so it is pinned here by checks that do not depend
on it: topological counts, the dof-count identity, a box it must reproduce, the patch test (a linear field is
annihilated on interior rows -- which proves the dofmaps conforming across blocks whose local axes disagree), the exact
energy of a linear field, two independent oracles against each other, and the partition's defining properties."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import multiblock_mesh as mb  # noqa: E402
from boundary_data_reference import twist  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

KAPPA = 2.0
GRAD = np.array([2.0, -3.0, 0.5])

# name -> (mesh, volume or None, affine cells)
_CATALOGUE = {}


def catalogue():
    if not _CATALOGUE:
        _CATALOGUE.update({
            "star3": (mb.star(3, 2, 2), 3 * np.sin(2 * np.pi / 3), True),
            "star5": (mb.star(5, 2, 3), 5 * np.sin(2 * np.pi / 5), True),
            "star3 bent": (mb.star(3, 2, 2, bend=0.3), 3 * np.sin(2 * np.pi / 3), False),
            "star5 bent": (mb.star(5, 2, 2, bend=0.3), 5 * np.sin(2 * np.pi / 5), False),
            "star4": (mb.star(4, 2, 2), 4.0, True),
            "ogrid": (mb.ogrid(2), 8.0, False),
            "ogrid twisted": (mb.ogrid(2, map=twist), None, False),
            "notched": (mb.notched((4, 3, 8)), None, True),
            "notched twisted": (mb.notched((3, 4, 8), map=twist), None, False),
        })
        nx = mb.notched_cells((4, 3, 8))
        _CATALOGUE["notched"] = (_CATALOGUE["notched"][0], len(nx) / (4 * 3 * 8), True)
    return _CATALOGUE


NAMES = ["star3", "star5", "star3 bent", "star5 bent", "star4", "ogrid", "ogrid twisted", "notched", "notched twisted"]


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_ogrid_counts():
    m = mb.ogrid(2)
    t = m.topology()
    assert m.ncells == 56 and t["V"] == 79 and int(m.left_handed().sum()) == 24
    assert dict(t["edge_valence"]) == {2: 48, 3: 40, 4: 114}
    assert dict(t["vertex_valence"]) == {3: 8, 4: 26, 6: 20, 8: 25}
    # Euler characteristic of a ball
    assert t["V"] - t["E"] + t["F"] - t["C"] == 1
    assert len(t["exterior"][0]) == 6 * 4


@pytest.mark.parametrize("k,nz", [(3, 2), (5, 3), (4, 2)])
def test_star_counts(k, nz):
    m = mb.star(k, 2, nz)
    t = m.topology()
    assert m.ncells == 4 * k * nz and not m.left_handed().any()
    assert t["V"] - t["E"] + t["F"] - t["C"] == 1
    if k != 4:
        # the axis: nz edges shared by k cells; its inner vertices lie on 2k cells, its two ends on k
        assert t["edge_valence"][k] == nz
        assert t["vertex_valence"][2 * k] == nz - 1
        assert t["vertex_valence"][k] == 2
    else:
        assert set(t["edge_valence"]) == {1, 2, 4} and set(t["vertex_valence"]) == {1, 2, 4, 8}


def test_notched_counts():
    n = (4, 3, 8)
    m = mb.notched(n)
    cc = mb.notched_cells(n)
    assert m.ncells == len(cc) == 4 * 3 * 8 - 2 * 1 * 2 - 1
    t = m.topology()
    # a ball with one cavity
    assert t["V"] - t["E"] + t["F"] - t["C"] == 2
    # re-entrant edges (3 cells) and corners exist, and a boundary vertex lies strictly inside the bounding box
    assert t["edge_valence"][3] > 0 and t["vertex_valence"][7] > 0
    marker = m.boundary_marker(1).astype(bool)
    x = m.dof_coordinates(1)
    inside = ((x > 1e-9) & (x < 1 - 1e-9)).all(axis=1)
    assert (marker & inside).any()
    # columns of cells that stop and resume
    col = cc[(cc[:, 0] == 3) & (cc[:, 1] == 2)][:, 2]
    assert len(col) < 8 and col.min() == 0 and col.max() == 7


@pytest.mark.parametrize("name", NAMES)
def test_dof_count_identity(name):
    m = catalogue()[name][0]
    t = m.topology()
    for P in range(1, 9):
        n = m.ndofs(P)
        assert n == t["V"] + t["E"] * (P - 1) + t["F"] * (P - 1) ** 2 + t["C"] * (P - 1) ** 3
        dm = m.dofmap(P)
        assert dm.dtype == np.int32 and dm.shape == (m.ncells, (P + 1) ** 3)
        assert np.array_equal(np.unique(dm), np.arange(n))
    # the marker is the dofs of the faces counted once
    cells, facets = m.exterior_facets()
    for P in (1, 3):
        want = np.zeros(m.ndofs(P), dtype=bool)
        for c, f in zip(cells, facets):
            want[m.dofmap(P)[c, mb.facet_nodes(P, f)]] = True
        assert np.array_equal(m.boundary_marker(P).astype(bool), want)
        pts = m.facet_point_coordinates(P, cells, facets)
        assert pts.shape == (len(cells), (P + 1) ** 2, 3)


@pytest.mark.parametrize("P", [1, 2, 3])
def test_star4_is_the_box(P):
    """star(4) is the box [-1, 1]^2 x [0, h]: after matching dofs by coordinates the assembled matrices are equal."""
    h = 0.75
    m = mb.star(4, 2, 3, h=h)
    box = po.BoxMesh((4, 4, 3), lo=(-1.0, -1.0, 0.0), hi=(1.0, 1.0, h))
    assert m.ncells == box.ncells and m.ndofs(P) == box.ndofs(P)
    dist, to_box = cKDTree(box.dof_coordinates(P)).query(m.dof_coordinates(P))
    assert dist.max() < 1e-12 and np.array_equal(np.sort(to_box), np.arange(box.ndofs(P)))
    assert np.array_equal(box.boundary_marker(P)[to_box], m.boundary_marker(P))
    kappa = 2.0
    A = po.Laplacian(P, kappa, m.dofmap(P), m.xgeom, m.geom_dofmap, m.boundary_marker(P)).assemble_csr()
    B = po.Laplacian(P, kappa, box.dofmap(P), box.xgeom, box.geom_dofmap, box.boundary_marker(P)).assemble_csr()
    B = B[to_box][:, to_box]
    diff = abs(A - B)
    assert (diff.max() if diff.nnz else 0.0) <= 1e-13 * abs(B).max()


@pytest.mark.parametrize("name", NAMES)
def test_patch_test_and_energy(name):
    """A u = 0 on interior rows for a linear u, and u^T A u = kappa |grad u|^2 volume.  P = 1 on affine cells only: the
    2-point rule is not exact on a frustum."""
    m, volume, affine = catalogue()[name]
    for P in (1, 2, 3, 4):
        if P == 1 and not affine:
            continue
        A = po.Laplacian(P, KAPPA, m.dofmap(P), m.xgeom, m.geom_dofmap, np.zeros(m.ndofs(P), dtype=np.int8))
        u = 1.0 + m.dof_coordinates(P) @ GRAD
        y = A.apply(u)
        interior = m.boundary_marker(P) == 0
        assert interior.any()
        scale = np.abs(A.diagonal()).max() * np.abs(u).max()
        assert np.abs(y[interior]).max() < 1e-13 * scale, (name, P)
        if volume is not None:
            assert abs(u @ y - KAPPA * GRAD @ GRAD * volume) < 1e-12 * KAPPA * GRAD @ GRAD * volume, (name, P)
        # symmetric, and equal to its own CSR
        v = np.random.default_rng(P).standard_normal(m.ndofs(P))
        w = np.random.default_rng(P + 10).standard_normal(m.ndofs(P))
        assert abs(w @ A.apply(v) - v @ A.apply(w)) < 1e-13 * np.abs(w).sum() * np.abs(A.apply(v)).max()
        if P <= 3:
            assert _relerr(A.assemble_csr() @ v, A.apply(v)) < 1e-13


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("name", NAMES)
def test_numpy_oracle_against_c_oracle(built, name, P):
    from oracle import c_oracle as co

    m = catalogue()[name][0]
    kappa = np.random.default_rng(3).uniform(0.5, 3.0, m.ncells)
    bc = m.boundary_marker(P)
    A = po.Laplacian(P, kappa, m.dofmap(P), m.xgeom, m.geom_dofmap, bc)
    C = co.CLevel(P, kappa, m.dofmap(P), m.xgeom, m.geom_dofmap, bc)
    u = np.random.default_rng(P).standard_normal(m.ndofs(P))
    assert _relerr(C.apply(u), A.apply(u)) < 1e-13
    assert _relerr(C.diag_inverse(), A.diag_inverse()) < 1e-13
    assert (A.detJ > 0).all()


@pytest.mark.parametrize("name", ["ogrid", "ogrid twisted", "star5 bent"])
def test_reference_modules_on_left_handed_cells(name):
    """The per-term reference modules on these meshes.  With K = I the tensor reference must give the oracle's tensor,
    left-handed cells included (tests/tensor_coefficient_reference.py divided by a signed det J: a negative-definite
    tensor on the 24 left-handed cells of the O-grid, which no box mesh of the suite has); with any K the operator is
    positive definite; the mass weights sum to the volume; the face weights to the area."""
    import reaction_reference as rr
    import tensor_coefficient_reference as tc
    from boundary_data_reference import facet_geometry

    m, volume, _ = catalogue()[name]
    P = 2
    ident = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (m.ncells, 1))
    nomark = np.zeros(m.ndofs(P), dtype=np.int8)
    A = tc.laplacian(P, 1.0, m.dofmap(P), m.xgeom, m.geom_dofmap, nomark)
    assert _relerr(tc.tensor_G(P, m.xgeom, m.geom_dofmap, ident), A.G) < 1e-13
    tc.with_tensor(A, tc.random_spd(m.ncells, 5))
    assert A.diagonal().min() > 0
    u = np.random.default_rng(1).standard_normal(m.ndofs(P))
    assert u @ A.apply(u) > 0
    if volume is not None:
        assert abs(rr.mass_weights(P, m.xgeom, m.geom_dofmap).sum() - volume) < 1e-13 * volume
    if name == "ogrid":
        cells, facets = m.exterior_facets()
        wds, normal = facet_geometry(m, P, cells, facets)
        assert abs(wds.sum() - 24.0) < 1e-12


def _prolongation_matrix(pc, pf, dmc, dmf, nc, nf):
    """P as a sparse matrix, from the cell matrices: every cell that holds a fine dof gives the same row."""
    M = po.interpolation_matrix_3d(pc, pf)
    rows = np.repeat(dmf, dmc.shape[1], axis=1).ravel()
    cols = np.tile(dmc, (1, dmf.shape[1])).ravel()
    vals = np.tile(M.ravel(), dmf.shape[0])
    S = sp.coo_matrix((vals, (rows, cols)), shape=(nf, nc)).tocsr()
    mult = np.bincount(dmf.ravel(), minlength=nf)
    return sp.diags(1.0 / mult) @ S


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (1, 3), (3, 6), (4, 8), (2, 5)])
@pytest.mark.parametrize("name", ["star3", "star5 bent", "ogrid twisted", "notched"])
def test_transfers(built, name, pc, pf):
    """Prolongation reproduces coarse polynomials (of the coarse degree in physical coordinates on affine cells, linear
    ones on every mesh), restriction is P^T; numpy and C oracle agree."""
    from oracle import c_oracle as co

    m, _, affine = catalogue()[name]
    dmc, dmf, nc, nf = m.dofmap(pc), m.dofmap(pf), m.ndofs(pc), m.ndofs(pf)
    ip = po.Interpolator(pc, pf, dmc, dmf, nc, nf)
    xc, xf = m.dof_coordinates(pc), m.dof_coordinates(pf)

    def poly(x):
        lin = 1.0 + x @ GRAD
        return lin ** pc + 0.5 * x[:, 0] * x[:, 2] ** (pc - 1) if affine else lin

    assert np.abs(ip.interpolate(poly(xc)) - poly(xf)).max() < 1e-12 * np.abs(poly(xf)).max()
    Pm = _prolongation_matrix(pc, pf, dmc.astype(np.int64), dmf.astype(np.int64), nc, nf)
    rng = np.random.default_rng(pc * 10 + pf)
    uc, uf = rng.standard_normal(nc), rng.standard_normal(nf)
    assert _relerr(ip.interpolate(uc), Pm @ uc) < 1e-13
    assert _relerr(ip.reverse_interpolate(uf), Pm.T @ uf) < 1e-13
    zero = np.zeros(m.ncells)
    Cc = co.CLevel(pc, 1.0 + zero, dmc, m.xgeom, m.geom_dofmap, m.boundary_marker(pc))
    Cf = co.CLevel(pf, 1.0 + zero, dmf, m.xgeom, m.geom_dofmap, m.boundary_marker(pf))
    J = co.CInterp(Cc, Cf)
    assert _relerr(J.interpolate(uc), ip.interpolate(uc)) < 1e-13
    assert _relerr(J.reverse_interpolate(uf), ip.reverse_interpolate(uf)) < 1e-13


# ---- partitions: the irregular edge lies on the interface (the star's sectors are split between the ranks) --------------
def sector_owner(mesh, ranks):
    """Sector s of a star goes to rank s * ranks // k."""
    k = int(mesh.cell_block.max()) + 1
    return mesh.cell_block * ranks // k


PARTITIONS = [("star3", 3, 2), ("star3", 3, 3), ("star5 bent", 5, 2), ("star5 bent", 5, 3)]


@pytest.mark.parametrize("name,k,ranks", PARTITIONS)
def test_partition(built, name, k, ranks):
    m = catalogue()[name][0]
    owner = sector_owner(m, ranks)
    assert set(owner.tolist()) == set(range(ranks))
    parts = [m.partition(owner, r) for r in range(ranks)]
    for p in parts:
        # owned cells first, then every cell that shares a dof with an owned dof; the axis cells of other ranks among them
        assert np.array_equal(owner[p.cells[: p.ncells_owned]], np.full(p.ncells_owned, p.rank))
        assert (owner[p.cells[p.ncells_owned:]] != p.rank).all() and len(np.unique(p.cells)) == p.ncells
    for P in (1, 2, 4):
        n = m.ndofs(P)
        lvs = [p.level(P) for p in parts]
        # ownership is a partition of the dofs; the owner is the lowest rank of the cells on the dof
        owned = np.concatenate([lv.local_to_global[: lv.size_local] for lv in lvs])
        assert np.array_equal(np.sort(owned), np.arange(n))
        down = m.dof_owner(P, owner)
        for r, lv in enumerate(lvs):
            assert (down[lv.local_to_global[: lv.size_local]] == r).all()
            assert np.array_equal(down[lv.local_to_global[lv.size_local:]], lv.ghost_owners)
            assert lv.neighbors == sorted(lv.neighbors) and r not in lv.neighbors
            assert sum(lv.recv_counts) == lv.num_ghosts and sum(lv.send_counts) == len(lv.send_indices)
            # lcells / bcells as LevelData defines them
            ghost_cell = np.arange(parts[r].ncells) >= parts[r].ncells_owned
            mark = ghost_cell | (lv.dofmap >= lv.size_local).any(axis=1)
            assert np.array_equal(lv.lcells, np.nonzero(~mark)[0]) and np.array_equal(lv.bcells, np.nonzero(mark)[0])
            # every owned row is complete: all cells of the whole mesh on an owned dof are local
            on_owned = (down[m.dofmap(P)] == r).any(axis=1)
            assert set(np.nonzero(on_owned)[0].tolist()) <= set(parts[r].cells.tolist())
        # a forward scatter of a global vector reproduces it on every ghost
        g = np.random.default_rng(P).standard_normal(n)
        local = []
        for lv in lvs:
            v = np.full(lv.ndofs, np.nan)
            v[: lv.size_local] = g[lv.local_to_global[: lv.size_local]]
            local.append(v)
        for r, lv in enumerate(lvs):
            off = 0
            for i, q in enumerate(lv.neighbors):
                peer = lvs[q]
                j = peer.neighbors.index(r)
                assert peer.send_counts[j] == lv.recv_counts[i]
                s0 = sum(peer.send_counts[:j])
                buf = local[q][peer.send_indices[s0: s0 + peer.send_counts[j]]]
                local[r][lv.size_local + lv.recv_indices[off: off + lv.recv_counts[i]]] = buf
                off += lv.recv_counts[i]
        for lv, v in zip(lvs, local):
            assert np.array_equal(v, g[lv.local_to_global])
        # the sum over ranks of the locally assembled owned rows is the global operator
        kappa = np.random.default_rng(3).uniform(0.5, 3.0, m.ncells)
        A = po.Laplacian(P, kappa, m.dofmap(P), m.xgeom, m.geom_dofmap, m.boundary_marker(P))
        total = sp.csr_matrix((n, n))
        for p, lv in zip(parts, lvs):
            assert np.array_equal(lv.bc_marker, m.boundary_marker(P)[lv.local_to_global])
            Al = po.Laplacian(P, kappa[p.cells], lv.dofmap, p.xgeom, p.geom_dofmap, lv.bc_marker)
            if P <= 2:
                M = Al.assemble_csr().tocsr()[: lv.size_local].tocoo()
                total = total + sp.coo_matrix((M.data, (lv.local_to_global[M.row], lv.local_to_global[M.col])),
                                              shape=(n, n)).tocsr()
            y = Al.apply(g[lv.local_to_global])[: lv.size_local]
            assert _relerr(y, A.apply(g)[lv.local_to_global[: lv.size_local]]) < 1e-13
            # the rank's own coordinates and exterior facets are the whole mesh's
            assert np.array_equal(p.dof_coordinates(P), m.dof_coordinates(P)[lv.local_to_global])
            fc, ff = p.exterior_facets()
            gc, gf = m.exterior_facets()
            assert set(zip(p.cells[fc].tolist(), ff.tolist())) == {(c, f) for c, f in zip(gc.tolist(), gf.tolist())
                                                                   if c in set(p.cells.tolist())}
        if P <= 2:
            ref = A.assemble_csr()
            diff = abs(total - ref)
            assert (diff.max() if diff.nnz else 0.0) <= 1e-13 * abs(ref).max()
