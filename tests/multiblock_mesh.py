"""Multi-block hexahedral meshes for the tests: what an unstructured mesh hands the library and a box never does.

Every mesh is a union of blocks, each the trilinear image of a structured ``mx x my x mz`` grid; vertices that coincide
are merged, so blocks meet conformingly with local axes that need not line up.  That gives edges shared by 3 or 5 cells,
vertices of valence 3, 4, 6 and 10, left-handed cells, re-entrant corners and holes.  Plain numpy / scipy: nothing here
comes from the library or the oracles, which see only the arrays ``(dofmap, xgeom, geom_dofmap, bc_marker)``.

The dofmap of degree P is built by POSITION: the GLL nodes of every cell are mapped through the cell's trilinear map and
points closer than a tolerance tied to the shortest edge become one dof.  It is verified by COUNTING: the number of dofs
must be ``V + E (P-1) + F (P-1)^2 + C (P-1)^3`` with V, E, F, C counted topologically from ``geom_dofmap``.

Conventions (the project's): vertex ``i*4 + j*2 + k`` of a cell, cell-local node ``t = (a*nd + b)*nd + c`` with ``a``
along local axis 0, local facet ``2*axis + side``."""
from __future__ import annotations

from collections import Counter

import numpy as np
from numpy.polynomial import legendre as _leg
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

# the 12 edges and 6 faces of a cell as local vertex numbers i*4 + j*2 + k
_EDGES = np.array([(v, v | b) for b in (4, 2, 1) for v in range(8) if not v & b])
_FACES = np.array([[v for v in range(8) if ((v >> (2 - axis)) & 1) == side] for axis in range(3) for side in range(2)])


def gll_nodes(nd: int) -> np.ndarray:
    """The nd Gauss-Lobatto-Legendre nodes on [0, 1], ascending, exactly symmetric about 1/2."""
    if nd == 2:
        return np.array([0.0, 1.0])
    c = np.zeros(nd)
    c[-1] = 1.0
    d1, d2 = _leg.legder(c), _leg.legder(c, 2)
    x = np.sort(_leg.legroots(d1))
    for _ in range(3):
        x = x - _leg.legval(x, d1) / _leg.legval(x, d2)
    x = np.concatenate(([-1.0], x, [1.0]))
    x = 0.5 * (x - x[::-1])
    return 0.5 * (x + 1.0)


def facet_nodes(P: int, local_facet: int) -> np.ndarray:
    """The nd*nd cell-local nodes of the face ``2*axis + side``, ordered by the two remaining axes ascending."""
    nd = P + 1
    axis, side = divmod(int(local_facet), 2)
    idx = [np.arange(nd)] * 3
    idx[axis] = np.array([P if side else 0])
    a, b, c = np.meshgrid(*idx, indexing="ij")
    return ((a * nd + b) * nd + c).ravel()


def _shape_matrix(P: int) -> np.ndarray:
    """[nd^3, 8]: the trilinear vertex functions at the cell's GLL nodes."""
    xi = gll_nodes(P + 1)
    phi = np.stack([1.0 - xi, xi], axis=1)
    return np.einsum("ai,bj,cl->abcijl", phi, phi, phi).reshape((P + 1) ** 3, 8)


def _cluster(points: np.ndarray, tol: float):
    """Labels of the clusters of points closer than ``tol`` (transitively), numbered by first appearance."""
    n = len(points)
    pairs = cKDTree(points).query_pairs(tol, output_type="ndarray")
    g = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    _, first = np.unique(lab, return_index=True)
    new = np.empty(ncomp, dtype=np.int64)
    new[np.argsort(first)] = np.arange(ncomp)
    return new[lab], ncomp


class _Cells:
    """What the library's partition object offers, over a list of cells of a mesh with a local dof numbering
    (``_numbering``): shared by the whole mesh (one rank) and a rank's share of it."""

    def level(self, P: int):
        raise NotImplementedError

    def dof_coordinates(self, P: int) -> np.ndarray:
        lv = self.level(P)
        if lv.dof_coords is None:
            pts = np.einsum("tk,ckd->ctd", _shape_matrix(P), self.xgeom[self.geom_dofmap])
            out = np.zeros((lv.ndofs, 3))
            out[lv.dofmap.ravel()] = pts.reshape(-1, 3)
            lv.dof_coords = out
        return lv.dof_coords

    def facet_point_coordinates(self, P: int, cells, local_facets) -> np.ndarray:
        """[nfacets, nd*nd, 3], in each cell's own frame, in the order of ``facet_nodes``."""
        nd = P + 1
        cells, local_facets = np.asarray(cells, dtype=np.int64), np.asarray(local_facets, dtype=np.int64)
        if cells.size == 0:
            return np.zeros((0, nd * nd, 3))
        nodes = np.stack([facet_nodes(P, f) for f in range(6)])
        return self.dof_coordinates(P)[self.level(P).dofmap[cells[:, None], nodes[local_facets]]]


class MultiblockMesh(_Cells):
    def __init__(self, xgeom, geom_dofmap, cell_block=None):
        self.xgeom = np.ascontiguousarray(xgeom, dtype=np.float64)
        self.geom_dofmap = np.ascontiguousarray(geom_dofmap, dtype=np.int32)
        self.ncells = self.geom_dofmap.shape[0]
        self.cell_block = np.zeros(self.ncells, dtype=np.int64) if cell_block is None else np.asarray(cell_block)
        e = self.xgeom[self.geom_dofmap[:, _EDGES]]
        self.shortest_edge = float(np.linalg.norm(e[:, :, 1] - e[:, :, 0], axis=2).min())
        self._dofmaps, self._levels, self._topology = {}, {}, None

    # ---- topology, counted from geom_dofmap alone ----
    def topology(self) -> dict:
        """V, E, F, C; the number of cells on every edge and vertex (``edge_valence`` / ``vertex_valence``: Counters
        valence -> how many); the exterior faces (those counted once) as ``(cells, local_facets)``."""
        if self._topology is None:
            gd = self.geom_dofmap.astype(np.int64)
            _, ecount = np.unique(np.sort(gd[:, _EDGES].reshape(-1, 2), axis=1), axis=0, return_counts=True)
            _, finv, fcount = np.unique(np.sort(gd[:, _FACES].reshape(-1, 4), axis=1), axis=0, return_inverse=True,
                                        return_counts=True)
            vcount = np.bincount(gd.ravel(), minlength=len(self.xgeom))
            assert vcount.min() > 0 and fcount.max() <= 2
            ext = np.nonzero(fcount[finv.ravel()] == 1)[0]  # (ordered by cell, then facet)
            self._topology = dict(V=len(self.xgeom), E=len(ecount), F=len(fcount), C=self.ncells,
                                  edge_valence=Counter(ecount.tolist()), vertex_valence=Counter(vcount.tolist()),
                                  exterior=((ext // 6).astype(np.int32), (ext % 6).astype(np.int8)))
        return self._topology

    def expected_ndofs(self, P: int) -> int:
        t = self.topology()
        return t["V"] + t["E"] * (P - 1) + t["F"] * (P - 1) ** 2 + t["C"] * (P - 1) ** 3

    def left_handed(self) -> np.ndarray:
        """bool [ncells]: det J < 0 at the cell's centre."""
        x = self.xgeom[self.geom_dofmap]
        J = np.stack([x[:, _FACES[2 * a + 1]].mean(axis=1) - x[:, _FACES[2 * a]].mean(axis=1) for a in range(3)], axis=2)
        return np.linalg.det(J) < 0

    def exterior_facets(self):
        return self.topology()["exterior"]

    # ---- function spaces ----
    def dofmap(self, P: int) -> np.ndarray:
        if P not in self._dofmaps:
            N = (P + 1) ** 3
            pts = np.einsum("tk,ckd->ctd", _shape_matrix(P), self.xgeom[self.geom_dofmap]).reshape(-1, 3)
            lab, n = _cluster(pts, 1e-7 * self.shortest_edge)
            dm = lab.reshape(self.ncells, N)
            if n != self.expected_ndofs(P):
                raise RuntimeError(f"degree {P}: {n} dofs by position, {self.expected_ndofs(P)} by counting")
            if (np.diff(np.sort(dm, axis=1), axis=1) == 0).any():
                raise RuntimeError(f"degree {P}: two nodes of one cell were merged")
            self._dofmaps[P] = np.ascontiguousarray(dm, dtype=np.int32)
        return self._dofmaps[P]

    def ndofs(self, P: int) -> int:
        return int(self.dofmap(P).max()) + 1

    global_ndofs = ndofs

    def boundary_marker(self, P: int) -> np.ndarray:
        """int8, 1 on every dof of an exterior face."""
        cells, facets = self.exterior_facets()
        nodes = np.stack([facet_nodes(P, f) for f in range(6)])
        m = np.zeros(self.ndofs(P), dtype=np.int8)
        m[self.dofmap(P)[cells.astype(np.int64)[:, None], nodes[facets.astype(np.int64)]]] = 1
        return m

    def level(self, P: int):
        from pmg_dolfinx_amd.mesh import LevelData

        if P not in self._levels:
            n, none = self.ndofs(P), np.zeros(0, dtype=np.int32)
            self._levels[P] = LevelData(
                P=P, size_local=n, num_ghosts=0, dofmap=self.dofmap(P), bc_marker=self.boundary_marker(P),
                local_to_global=np.arange(n, dtype=np.int64), ghost_owners=none, neighbors=[], send_counts=[],
                recv_counts=[], send_indices=none, recv_indices=none, lcells=np.arange(self.ncells, dtype=np.int32),
                bcells=none)
        return self._levels[P]

    # ---- partition ----
    def dof_owner(self, P: int, cell_owner) -> np.ndarray:
        """The lowest owning rank of the cells on every dof."""
        dm = self.dofmap(P)
        own = np.full(self.ndofs(P), np.iinfo(np.int64).max)
        np.minimum.at(own, dm.ravel(), np.repeat(np.asarray(cell_owner, dtype=np.int64), dm.shape[1]))
        return own

    def rank_cells(self, cell_owner, rank: int):
        """(cells, number owned): the rank's own cells, then every other cell that shares a dof with a dof the rank
        owns.  Decided at degree 2, where every vertex, edge, face and cell carries a dof, so the list serves every
        degree."""
        cell_owner = np.asarray(cell_owner)
        touches = (self.dof_owner(2, cell_owner)[self.dofmap(2)] == rank).any(axis=1)
        owned = np.nonzero(cell_owner == rank)[0]
        ghost = np.nonzero(touches & (cell_owner != rank))[0]
        return np.concatenate([owned, ghost]), len(owned)

    def partition(self, cell_owner, rank: int) -> "RankPart":
        return RankPart(self, np.asarray(cell_owner, dtype=np.int64), int(rank))


class RankPart(_Cells):
    """One rank's share: ``cells`` (global numbers: owned, then ghost), the geometry rows of those cells over the whole
    mesh's ``xgeom``, and per degree a ``LevelData`` with owned dofs first (ascending global number), then the ghosts
    grouped by owner (ascending global number inside a group); the halo lists are grouped by neighbour."""

    def __init__(self, mesh: MultiblockMesh, cell_owner, rank: int):
        self.mesh, self.cell_owner, self.rank = mesh, cell_owner, rank
        self.size = int(cell_owner.max()) + 1
        self.cells, self.ncells_owned = mesh.rank_cells(cell_owner, rank)
        self.ncells = len(self.cells)
        self.xgeom = mesh.xgeom
        self.geom_dofmap = np.ascontiguousarray(mesh.geom_dofmap[self.cells])
        self._levels = {}

    def global_ndofs(self, P: int) -> int:
        return self.mesh.ndofs(P)

    def _local_dofs(self, P: int, rank: int):
        """Global numbers of a rank's local dofs in its local order, and how many of them it owns."""
        owner = self.mesh.dof_owner(P, self.cell_owner)
        cells = self.cells if rank == self.rank else self.mesh.rank_cells(self.cell_owner, rank)[0]
        g = np.unique(self.mesh.dofmap(P)[cells])
        mine, ghosts = g[owner[g] == rank], g[owner[g] != rank]
        ghosts = ghosts[np.lexsort((ghosts, owner[ghosts]))]
        return np.concatenate([mine, ghosts]), len(mine), owner

    def level(self, P: int):
        from pmg_dolfinx_amd.mesh import LevelData

        if P in self._levels:
            return self._levels[P]
        l2g, size_local, owner = self._local_dofs(P, self.rank)
        g2l = np.full(self.mesh.ndofs(P), -1, dtype=np.int64)
        g2l[l2g] = np.arange(len(l2g))
        dofmap = np.ascontiguousarray(g2l[self.mesh.dofmap(P)[self.cells]], dtype=np.int32)
        assert dofmap.min() >= 0
        ghost_owners = owner[l2g[size_local:]]
        neighbors, send_counts, recv_counts, send_lists = [], [], [], []
        for q in range(self.size):
            if q == self.rank:
                continue
            gq, nq, _ = self._local_dofs(P, q)
            send = gq[nq:][owner[gq[nq:]] == self.rank]  # q's ghosts that this rank owns, in q's ghost order
            nrecv = int((ghost_owners == q).sum())
            if len(send) == 0 and nrecv == 0:
                continue
            neighbors.append(q)
            send_counts.append(len(send))
            recv_counts.append(nrecv)
            send_lists.append(g2l[send])
        ghost_cell = np.arange(self.ncells) >= self.ncells_owned
        mark = ghost_cell | (dofmap >= size_local).any(axis=1)
        lv = LevelData(
            P=P, size_local=size_local, num_ghosts=len(l2g) - size_local, dofmap=dofmap,
            bc_marker=np.ascontiguousarray(self.mesh.boundary_marker(P)[l2g]), local_to_global=l2g,
            ghost_owners=ghost_owners.astype(np.int32), neighbors=neighbors, send_counts=send_counts,
            recv_counts=recv_counts,
            send_indices=(np.concatenate(send_lists) if send_lists else np.zeros(0)).astype(np.int32),
            recv_indices=np.arange(len(l2g) - size_local, dtype=np.int32),
            lcells=np.nonzero(~mark)[0].astype(np.int32), bcells=np.nonzero(mark)[0].astype(np.int32))
        assert (lv.send_indices < size_local).all() and (lv.send_indices >= 0).all()
        self._levels[P] = lv
        return lv

    def exterior_facets(self):
        """The whole mesh's exterior faces that belong to a local cell (ghost cells included), by local cell number."""
        cells, facets = self.mesh.exterior_facets()
        local = np.full(self.mesh.ncells, -1, dtype=np.int64)
        local[self.cells] = np.arange(self.ncells)
        keep = local[cells] >= 0
        lc, lf = local[cells[keep]], facets[keep]
        order = np.lexsort((lf, lc))
        return lc[order].astype(np.int32), lf[order].astype(np.int8)


# ---- construction ---------------------------------------------------------------------------------------------------
def from_blocks(corners, m=(1, 1, 1), map=None) -> MultiblockMesh:  # noqa: A002 (the issue's name of the argument)
    """``corners[nb, 8, 3]``: block vertices in the order ``i*4 + j*2 + k``; every block becomes the trilinear image of a
    structured ``mx x my x mz`` grid, cells lexicographic (local axis 0 slowest); coinciding vertices are merged; ``map``
    (a smooth map of points ``[n, 3]``) is applied to the merged vertices afterwards."""
    corners = np.asarray(corners, dtype=np.float64).reshape(-1, 8, 3)
    mx, my, mz = (int(v) for v in ((m,) * 3 if np.isscalar(m) else m))
    t = [np.linspace(0.0, 1.0, n + 1) for n in (mx, my, mz)]
    phi = [np.stack([1.0 - s, s], axis=1) for s in t]
    N = np.einsum("ai,bj,cl->abcijl", phi[0], phi[1], phi[2]).reshape(-1, 8)  # [(mx+1)(my+1)(mz+1), 8]
    pts = np.einsum("vk,bkd->bvd", N, corners)
    nv = pts.shape[1]
    ci, cj, ck = (a.ravel() for a in np.meshgrid(np.arange(mx), np.arange(my), np.arange(mz), indexing="ij"))
    gd = np.stack([((ci + i) * (my + 1) + cj + j) * (mz + 1) + ck + k for i in range(2) for j in range(2)
                   for k in range(2)], axis=1)
    gd = (gd[None] + nv * np.arange(len(corners))[:, None, None]).reshape(-1, 8)
    flat = pts.reshape(-1, 3)
    edges = flat[gd[:, _EDGES]]
    shortest = np.linalg.norm(edges[:, :, 1] - edges[:, :, 0], axis=2).min()
    lab, n = _cluster(flat, 1e-7 * shortest)
    x = np.zeros((n, 3))
    x[lab] = flat
    if map is not None:
        x = map(x)
    return MultiblockMesh(x, lab[gd], np.repeat(np.arange(len(corners)), mx * my * mz))


def star(k: int, m=2, nz: int = 2, bend: float = 0.0, h: float = 1.0) -> MultiblockMesh:
    """``k`` rhombic sectors (0, a_s, a_s + a_{s+1}, a_{s+1}), a_s = (cos 2 pi s/k, sin 2 pi s/k), around the z axis,
    ``m x m`` cells each, extruded over [0, h] in ``nz`` layers.  The axis is an edge shared by ``k`` cells with vertices
    of valence ``2k``; k = 4 is the box [-1, 1]^2 x [0, h].  ``bend = 0``: affine, sheared cells with one Jacobian per
    sector; ``bend > 0`` (x += bend z y): trilinear cells, the same volume ``k sin(2 pi/k) h``."""
    a = [np.array([np.cos(2 * np.pi * s / k), np.sin(2 * np.pi * s / k), 0.0]) for s in range(k + 1)]
    corners = np.array([[i * a[s] + j * a[s + 1] + np.array([0.0, 0.0, kz * h]) for i in range(2) for j in range(2)
                         for kz in range(2)] for s in range(k)])

    def bent(x):
        y = x.copy()
        y[:, 0] += bend * x[:, 2] * x[:, 1]
        return y

    mm = (m, m, nz) if np.isscalar(m) else m
    return from_blocks(corners, mm, map=bent if bend else None)


def ogrid(m=2, r: float = 0.4, map=None) -> MultiblockMesh:  # noqa: A002
    """The cube [-1, 1]^3 as an inner cube [-r, r]^3 plus six frustum blocks whose local axis 0 is radial.  Three of
    the frusta are left-handed and stay so."""
    def cube(s):
        return [[(2 * i - 1) * s, (2 * j - 1) * s, (2 * k - 1) * s] for i in range(2) for j in range(2) for k in range(2)]

    corners = [cube(r)]
    for axis in range(3):
        b, c = [a for a in range(3) if a != axis]
        for sign in (-1.0, 1.0):
            blk = []
            for i in range(2):
                s = r if i == 0 else 1.0
                for j in range(2):
                    for k in range(2):
                        p = [0.0] * 3
                        p[axis], p[b], p[c] = sign * s, (2 * j - 1) * s, (2 * k - 1) * s
                        blk.append(p)
            corners.append(blk)
    return from_blocks(np.array(corners), m, map=map)


def notched_cells(n):
    """The kept cells of ``notched(n)``, [ncells, 3] grid coordinates, lexicographic."""
    nx, ny, nz = n
    i, j, k = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"))
    notch = (i >= (nx + 1) // 2) & (j >= (ny + 1) // 2) & (k >= nz // 4) & (k < nz // 2)
    hole = (i == 1) & (j == 1) & (k == (3 * nz) // 4)
    keep = ~(notch | hole)
    return np.stack([i[keep], j[keep], k[keep]], axis=1)


def notched(n, map=None) -> MultiblockMesh:  # noqa: A002
    """The ``nx x ny x nz`` grid of the unit box with a re-entrant notch cut from one vertical edge (columns of cells
    that stop and resume) and one interior cell removed: a tensor grid of centroids with gaps, with boundary dofs in the
    middle of the bounding box.  Every cell is a block of its own.  Needs nx, ny >= 3 and nz >= 4."""
    n = tuple(int(v) for v in n)
    assert n[0] >= 3 and n[1] >= 3 and n[2] >= 4
    cc = notched_cells(n)
    h = 1.0 / np.array(n)
    corners = np.array([[(c + np.array([i, j, k])) * h for i in range(2) for j in range(2) for k in range(2)]
                        for c in cc])
    return from_blocks(corners, 1, map=map)
