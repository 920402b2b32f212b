"""The driver-side wiring of ``examples/pmg/main.cpp:solve`` (``:41-380``) for a
structured box: per level function space data, operator, inverse diagonal, load
vector, eigenvalue estimate, Chebyshev smoother; the interpolators and the
V-cycle.  Generalised from the example's two levels {1, 3} to any ascending list
of degrees (BASELINE config 2 is {1, 2, 4})."""
from __future__ import annotations

import numpy as np

from .cg import CGSolver
from .chebyshev import Chebyshev
from .interpolate import Interpolator
from .laplacian import MatFreeLaplacian
from .matrix import MatrixOperator
from .mesh import BoxPartition, basix_node_permutation, default_proc_dims, dofmap_in_node_order
from .pmg import MultigridPreconditioner
from .vector import Layout, Vector


def make_layout(lv, group=None, device="cuda", comm=None) -> Layout:
    return Layout(lv.size_local, lv.num_ghosts, lv.neighbors, lv.send_counts, lv.recv_counts, lv.send_indices,
                  lv.recv_indices, group=group, device=device, comm=comm)


class PoissonHierarchy:
    def __init__(self, n, orders=(1, 2, 4), kappa=2.0, cheb_its=3, proc_dims=None, rank=0, size=1, group=None,
                 warp=None, eig_cg_its=20, eig_cg_rtol=1e-6, freq=(2, 3, 4), device="cuda", comm=None,
                 node_order="ascending", level_hook=None, assembled_levels=(), kappa_field=None, dirichlet=None,
                 kappa_tensor=None, reaction=None, robin=None, cell_frames=None, part=None, geom_degree=1):
        """``kappa_field`` (optional): a callable mapping dof coordinates ``[n, 3]`` to positive nodal values of a
        variable coefficient; it is evaluated on every level at that level's dof coordinates and set on the level's
        operator (``MatFreeLaplacian.set_coefficient_field``) before the diagonal and the eigenvalue estimate.  The
        load vectors keep the per-cell ``kappa`` only (``pmg_laplacian_assemble_rhs``).

        ``kappa_tensor`` (optional): a callable mapping cell centres ``[ncells, 3]`` (the mean of a cell's eight
        vertices) to ``[ncells, 6]``, one symmetric positive-definite diffusion tensor per cell as
        (xx, xy, xz, yy, yz, zz); it is set on every level's operator
        (``MatFreeLaplacian.set_coefficient_tensor``) beside ``kappa_field``, before the diagonal and the eigenvalue
        estimate.

        ``reaction`` (optional): a callable mapping cell centres ``[ncells, 3]`` to ``[ncells]``, one reaction
        coefficient sigma >= 0 per cell; every level's operator becomes -div(K grad u) + sigma u
        (``MatFreeLaplacian.set_reaction``), set next to ``kappa_tensor``, before the diagonal and the eigenvalue
        estimate.

        ``robin`` (optional): a callable mapping facet-point coordinates ``[n, 3]`` to ``alpha >= 0``, the coefficient
        of a Robin boundary term K grad u . n + alpha u = g.  It is evaluated on every level at that level's facet
        points of ``part.exterior_facets()`` and set on the level's operator (``MatFreeLaplacian.set_robin``) next to
        ``reaction``, before the diagonal and the eigenvalue estimate; marked dofs carry none, so together with
        ``dirichlet`` it describes the whole problem (a problem without any Dirichlet dof included).  The data g
        enters the caller's right-hand side through ``assemble_neumann``.

        ``dirichlet`` (optional): a callable mapping dof coordinates ``[n, 3]`` to a boolean array; on every level
        the Dirichlet marker becomes the exterior dofs for which it is true (default: the whole boundary).  The rest
        of the boundary is natural; non-zero data enter through ``MatFreeLaplacian.apply_lifting`` / ``set_bc`` /
        ``assemble_neumann`` on the caller's right-hand side.

        ``cell_frames`` (optional): every cell's local frame, an int array over the global cell grid
        (``BoxPartition``); the problem and its solution do not depend on it.

        ``part`` (optional): this rank's share of any conforming hexahedral mesh, an object with ``BoxPartition``'s
        members (``xgeom``, ``geom_dofmap``, ``ncells``, ``level(P)``, ``dof_coordinates(P)``, ``exterior_facets()``,
        ``facet_point_coordinates(P, cells, facets)``), used instead of constructing one; ``n``, ``proc_dims``,
        ``rank``, ``size``, ``warp``, ``cell_frames`` and ``geom_degree`` are then ignored.  Such a mesh announces the
        degree of its coordinate element through an attribute ``geom_degree`` (1 when absent).

        ``geom_degree`` (1..4): the degree g of the coordinate element (``BoxPartition``); ``warp`` is evaluated at the
        degree-g nodes of every cell."""
        import torch

        self.orders = tuple(int(p) for p in orders)
        if list(self.orders) != sorted(set(self.orders)):
            raise ValueError("orders must be strictly ascending (coarse -> fine)")
        dims = tuple(proc_dims) if proc_dims is not None else default_proc_dims(size)
        self.part = part if part is not None else BoxPartition(n, dims, rank, warp=warp, cell_frames=cell_frames,
                                                                   geom_degree=geom_degree)
        part = self.part
        self.geom_degree = gdeg = int(getattr(part, "geom_degree", 1))
        # the 8 corners among a cell's (g+1)^3 geometry nodes (cell centres: their mean)
        corners = [((i * gdeg * (gdeg + 1)) + j * gdeg) * (gdeg + 1) + k * gdeg
                   for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        self.levels, self.layouts, self.operators, self.smoothers, self.eig_ranges = [], [], [], [], []
        self.rhs = []
        dev = torch.device(device)
        # geometry is shared by all levels (examples/pmg/main.cpp:243-254)
        self.xgeom = torch.from_numpy(part.xgeom).to(dev)
        self.geom_dofmap = torch.from_numpy(part.geom_dofmap).to(dev)
        self.kappa = torch.full((part.ncells,), float(kappa), dtype=torch.float64, device=dev)  # :190-193
        # node_order = "basix": the dofmaps are handed over as dolfinx would hold them (endpoints first per direction)
        self.node_order = node_order
        ktensor = None
        if kappa_tensor is not None:  # the cells are the same on every level
            centres = part.xgeom[part.geom_dofmap[:, corners]].mean(axis=1)
            ktensor = torch.from_numpy(np.ascontiguousarray(kappa_tensor(centres), dtype=np.float64)).to(dev)
        sigma = None
        if reaction is not None:
            centres = part.xgeom[part.geom_dofmap[:, corners]].mean(axis=1)
            sigma = torch.from_numpy(np.ascontiguousarray(reaction(centres), dtype=np.float64).reshape(-1)).to(dev)
        for P in self.orders:
            lv = part.level(P)
            if level_hook is not None:  # bench.py --corrupt-halo: a deliberately wrong halo plan for the gate's own test
                level_hook(lv)
            if dirichlet is not None:
                keep = np.asarray(dirichlet(part.dof_coordinates(P)), dtype=bool)
                lv.bc_marker = (lv.bc_marker.astype(bool) & keep).astype(np.int8)
            layout = make_layout(lv, group, device, comm)
            dofmap = lv.dofmap
            if node_order in ("basix", "endpoints_first"):
                dofmap = dofmap_in_node_order(lv.dofmap, basix_node_permutation(P))
            elif node_order != "ascending":
                raise ValueError("PoissonHierarchy: node_order is 'ascending' or 'basix'")
            op = MatFreeLaplacian(P, self.kappa, dofmap, self.xgeom, self.geom_dofmap, lv.lcells, lv.bcells,
                                  lv.bc_marker, layout, node_order=node_order, geometry_degree=gdeg)  # :270-272
            if kappa_field is not None:
                kq = Vector(layout)
                kq.data.copy_(torch.from_numpy(np.ascontiguousarray(
                    kappa_field(part.dof_coordinates(P)), dtype=np.float64)))
                op.set_coefficient_field(kq)
                del kq
            if ktensor is not None:
                op.set_coefficient_tensor(ktensor)
            if sigma is not None:
                op.set_reaction(sigma)
            if robin is not None:
                fc, fl = part.exterior_facets()
                pts = part.facet_point_coordinates(P, fc, fl)
                alpha = np.ascontiguousarray(robin(pts.reshape(-1, 3)), dtype=np.float64).reshape(len(fc), -1)
                op.set_robin(fc, fl, alpha)
            op.compute_diag_inverse()  # replaces :274-279
            self.levels.append(lv)
            self.layouts.append(layout)
            self.operators.append(op)
            # load vector, :289-300 with f of examples/pmg/poisson.py:6-8,30
            c = part.dof_coordinates(P)
            kx, ky, kz = freq
            fvals = ((kx * kx + ky * ky + kz * kz) * np.pi**2 * np.sin(kx * np.pi * c[:, 0])
                     * np.sin(ky * np.pi * c[:, 1]) * np.sin(kz * np.pi * c[:, 2]))
            f = Vector(layout)
            f.data.copy_(torch.from_numpy(fvals))
            b = Vector(layout)
            op.assemble_rhs(f, b)
            self.rhs.append(b)
            del f
        # smoothers, :306-330
        for i, P in enumerate(self.orders):
            layout, op = self.layouts[i], self.operators[i]
            cg = CGSolver(layout)
            cg.set_max_iterations(eig_cg_its)
            cg.set_tolerance(eig_cg_rtol)
            cg.store_coefficients(True)
            x = Vector(layout)
            y = Vector(layout)
            x.set(0.0)
            y.set(1.0)
            cg.solve(op, x, y)
            eig = np.sort(cg.compute_eigenvalues())
            rng = (0.1 * eig[-1], 1.1 * eig[-1])  # :327
            sm = Chebyshev(layout, rng)
            sm.set_max_iterations(cheb_its)
            self.smoothers.append(sm)
            self.eig_ranges.append(rng)
            del cg, x, y
        # interpolators, :336-341
        self.interpolators = []
        for i in range(len(self.orders) - 1):
            lc, lf = self.levels[i], self.levels[i + 1]
            self.interpolators.append(
                Interpolator(self.orders[i], self.orders[i + 1], self.operators[i].dofmap,
                             self.operators[i + 1].dofmap, lf.lcells, lf.bcells, self.layouts[i],
                             self.layouts[i + 1], fine_operator=self.operators[i + 1], node_order=node_order))
        # V-cycle, :348-355
        self.mg = MultigridPreconditioner(self.layouts, self.levels[0].bc_marker)
        self.mg.set_solvers(self.smoothers)
        self.mg.set_operators(self.operators)
        self.mg.set_interpolators(self.interpolators)
        # assembled levels (solve<acc::MatrixOperator>, examples/pmg/main.cpp:285): opt-in, level by level
        self.matrices = {}
        for i in assembled_levels:
            i = int(i) % len(self.orders)
            # on several ranks the distributed form (ghost columns, diag / off-diag split)
            several = self.levels[i].num_ghosts > 0 or comm is not None or group is not None
            self.matrices[i] = MatrixOperator(self.operators[i], distributed=several)
            self.mg.set_level_matrix(i, self.matrices[i])

    @property
    def fine_ndofs_owned(self):
        return self.levels[-1].size_local

    def new_vector(self, level=-1):
        return Vector(self.layouts[level])
