"""Host mirror of ``acc::MatFreeLaplacian`` (``src/laplacian.hpp:284-526``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import call, current_stream, ptr, vp
from .vector import Layout, Vector


def _dev_i32(a, device):
    import torch

    if hasattr(a, "data_ptr"):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def _dev_f64(a, device):
    import torch

    if hasattr(a, "data_ptr"):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _dev_i8(a, device):
    import torch

    if hasattr(a, "data_ptr"):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int8)).to(device)


NODE_ORDERS = {"ascending": 0, "endpoints_first": 1, "basix": 1, "custom": 2}


def node_order_args(node_order, degree, perm1d=None):
    """(order code, int32 permutation or None) for the ``*_ordered`` entry points.  ``node_order`` is
    "ascending", "basix" / "endpoints_first" (vertex 0, vertex 1, interior left to right: the order of a
    basix tensor-product element, ``examples/pmg/main.cpp:83-87``) or "custom" with
    ``perm1d[j]`` = ascending position of the caller's 1-D node ``j``."""
    code = NODE_ORDERS[node_order] if isinstance(node_order, str) else int(node_order)
    perm = None
    if code == 2:
        perm = np.ascontiguousarray(perm1d, dtype=np.int32)
        if perm.size != degree + 1:
            raise ValueError("perm1d needs degree + 1 entries")
    return code, perm


def node_permutation(node_order, degree, perm1d=None):
    """perm1d[j] = ascending position of 1-D node j in the given order (``pmg_node_permutation``)."""
    code, perm = node_order_args(node_order, degree, perm1d)
    out = np.zeros(degree + 1, dtype=np.int32)
    call("pmg_node_permutation", code, int(degree), perm.ctypes.data_as(_lib.c_ip) if perm is not None else None,
         out.ctypes.data_as(_lib.c_ip))
    return out


def set_merge_threshold(patch_dofs: int):
    """Launch plan of operators created from now on: interior colours are merged into one atomic
    launch when the interior list has at most ``patch_dofs`` patch dofs (0: always coloured
    launches; negative: the library's measured defaults).  Process-wide; tests and tuning."""
    call("pmg_set_merge_threshold", int(patch_dofs))


class MatFreeLaplacian:
    """y = A x for the GLL-collocated stiffness operator, matrix-free.

    Argument order follows the reference constructor (``:289-297``); arrays may be
    numpy (uploaded here) or device torch tensors (used in place -- they must
    outlive the operator, exactly like the reference's non-owning spans).  The
    coordinate-element tabulation ``dphi_geometry`` and ``G_weights`` of the
    reference are derived from ``degree`` inside the library.
    """

    value_type = np.float64

    def __init__(self, degree, coefficients, dofmap, xgeom, geometry_dofmap, lcells, bcells, bc_marker,
                 layout: Layout, batch_size: int = 0, node_order="ascending", perm1d=None, dphi_geometry=None,
                 G_weights=None, geometry_degree: int = 1):
        """``geometry_degree`` g (1..4): the coordinate element is the tensor-product Lagrange element of degree g on
        the GLL nodes; ``geometry_dofmap`` is ``[ncells, (g+1)^3]`` in ascending tensor order (``include/pmg_amd.h``,
        "curved cells") and ``dphi_geometry``, when given, ``[3, nq, (g+1)^3]``."""
        if batch_size != 0:
            # src/laplacian.hpp:391-396 recomputes G per batch to save memory; with
            # 288 GB of HBM the tensor is always resident.
            raise ValueError("geometry batching is not supported: G is kept resident in HBM")
        dev = layout.device
        self.layout = layout
        self.degree = int(degree)
        N = (self.degree + 1) ** 3
        self.dofmap = _dev_i32(dofmap, dev)
        self.ncells = int(self.dofmap.numel() // N) if self.degree >= 1 else 0
        self.kappa = _dev_f64(np.broadcast_to(np.asarray(coefficients, dtype=np.float64), (self.ncells,)).copy()
                              if not hasattr(coefficients, "data_ptr") else coefficients, dev)
        self.xgeom = _dev_f64(xgeom, dev)
        self.geom_degree = int(geometry_degree)
        if not 1 <= self.geom_degree <= 4:
            raise ValueError(f"geometry_degree {geometry_degree} outside 1..4")
        ng = (self.geom_degree + 1) ** 3
        self.geom_dofmap = _dev_i32(geometry_dofmap, dev)
        supported = 1 <= self.degree <= 8  # (any other degree is the library's to refuse: "Unsupported degree")
        if supported and self.geom_dofmap.numel() != self.ncells * ng:
            raise ValueError(f"geometry_dofmap has {self.geom_dofmap.numel()} entries, {self.ncells} cells of geometry "
                             f"degree {self.geom_degree} need {self.ncells * ng}")
        if supported and dphi_geometry is not None and int(np.prod(tuple(dphi_geometry.shape))) != 3 * N * ng:
            raise ValueError(f"dphi_geometry has {int(np.prod(tuple(dphi_geometry.shape)))} entries, degree "
                             f"{self.degree} with geometry degree {self.geom_degree} needs {3 * N * ng}")
        self.bc_marker = _dev_i8(bc_marker, dev)
        if self.bc_marker.numel() != layout.total:
            raise ValueError("bc_marker must have size_local + num_ghosts entries")
        lc = np.ascontiguousarray(lcells, dtype=np.int32)
        bc_ = np.ascontiguousarray(bcells, dtype=np.int32)
        h = vp()
        # cell-local node order of `dofmap` (and of the two tables when given): the reference's arrays come from a
        # basix tensor-product element, i.e. "basix" (src/laplacian.hpp:289-297, examples/pmg/main.cpp:83-87)
        self.node_order, perm = node_order_args(node_order, self.degree, perm1d)
        self.dphi_geometry = _dev_f64(dphi_geometry, dev) if dphi_geometry is not None else None
        self.G_weights = _dev_f64(G_weights, dev) if G_weights is not None else None
        if (self.dphi_geometry is None) != (self.G_weights is None):
            raise ValueError("dphi_geometry and G_weights come together (src/laplacian.hpp:293-294)")
        call("pmg_laplacian_create_curved", C.byref(h), layout.handle, self.degree, self.ncells, ptr(self.kappa),
             ptr(self.dofmap), ptr(self.xgeom), int(self.xgeom.numel() // 3), self.geom_degree, ptr(self.geom_dofmap),
             ptr(self.dphi_geometry), ptr(self.G_weights),
             lc.ctypes.data_as(_lib.c_ip), lc.size, bc_.ctypes.data_as(_lib.c_ip), bc_.size, ptr(self.bc_marker),
             self.node_order, perm.ctypes.data_as(_lib.c_ip) if perm is not None else None, current_stream())
        self._handle = h
        # bumped by every method that changes a coefficient other than kappa (set_coefficient_field,
        # set_coefficient_tensor, set_reaction, set_robin), before the library is called: a refused call leaves the
        # count ahead, the safe side for adjoint.solve's staleness guard
        self.coefficient_epoch = 0

    @property
    def handle(self):
        return self._handle

    def geometry_degree(self) -> int:
        """Degree of the coordinate element the operator was created with (``pmg_laplacian_geometry_degree``)."""
        return int(call("pmg_laplacian_geometry_degree", self._handle))

    def __call__(self, x: Vector, y: Vector):  # operator()(in, out), :462-482
        call("pmg_laplacian_apply", self._handle, ptr(x.data), ptr(y.data), current_stream())

    def apply_fp32(self, x, y):
        """y = A x in FP32 (``pmg_laplacian_apply_f32``) on float32 device tensors of the layout's total size;
        y is overwritten.  Single domain only."""
        import torch

        n = self.layout.size_local + self.layout.num_ghosts
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"{name} must be a contiguous float32 torch tensor")
            if t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, the layout {n}")
        call("pmg_laplacian_apply_f32", self._handle, vp(x.data_ptr()), vp(y.data_ptr()), current_stream())

    def get_diag_inverse(self, diag_inv: Vector):  # :484-488
        call("pmg_laplacian_get_diag_inverse", self._handle, ptr(diag_inv.data), current_stream())

    def set_diag_inverse(self, diag_inv: Vector):  # :490-495
        call("pmg_laplacian_set_diag_inverse", self._handle, ptr(diag_inv.data), current_stream())

    def compute_diag_inverse(self):
        """Matrix-free replacement of the CSR detour of ``examples/pmg/main.cpp:274-279``."""
        call("pmg_laplacian_compute_diag_inverse", self._handle, current_stream())

    def set_coefficient_field(self, v):
        """Nodal coefficient kq (``pmg_laplacian_set_coefficient_field``): the operator becomes
        -div(kappa[cell] * kq(x) grad u).  ``v`` is a ``Vector`` of the operator's layout whose owned entries are
        the values at the dofs (all finite and > 0; its ghost entries are not read, the library scatters its own
        copy), or ``None`` to remove the field.  The tensor, its float form and a computed inverse diagonal are
        rebuilt; not inside a stream capture."""
        self.coefficient_epoch += 1
        if v is None:
            call("pmg_laplacian_set_coefficient_field", self._handle, None, current_stream())
            return
        if not isinstance(v, Vector):
            raise TypeError("set_coefficient_field takes a Vector of the operator's layout, or None")
        n = self.layout.size_local + self.layout.num_ghosts
        if v.data.numel() != n:
            raise ValueError(f"the field has {v.data.numel()} entries, the operator's layout {n}")
        call("pmg_laplacian_set_coefficient_field", self._handle, ptr(v.data), current_stream())

    def has_coefficient_field(self) -> bool:
        return bool(call("pmg_laplacian_has_coefficient_field", self._handle))

    def set_coefficient_tensor(self, t):
        """Per-cell diffusion tensor K (``pmg_laplacian_set_coefficient_tensor``): the operator becomes
        -div(kappa[cell] * kq(x) * K[cell] grad u).  ``t`` is a float64 numpy array (uploaded here) or torch tensor
        of shape ``(ncells, 6)``, one symmetric positive-definite tensor per local cell, ghost cells included, as
        (xx, xy, xz, yy, yz, zz) in physical coordinates; or ``None`` to remove the tensor.  The library copies it.
        The stored tensor, its float and affine forms and a computed inverse diagonal are rebuilt; not inside a
        stream capture."""
        self.coefficient_epoch += 1
        import torch

        if t is None:
            call("pmg_laplacian_set_coefficient_tensor", self._handle, None, current_stream())
            return
        if not isinstance(t, (np.ndarray, torch.Tensor)):
            raise TypeError("set_coefficient_tensor takes a float64 numpy array or torch tensor, or None")
        if t.dtype not in (np.float64, torch.float64):
            raise TypeError(f"the coefficient tensor must be float64, not {t.dtype}")
        if tuple(t.shape) != (self.ncells, 6):
            raise ValueError(f"the coefficient tensor has shape {tuple(t.shape)}, the operator needs "
                             f"({self.ncells}, 6)")
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        t = t.to(self.layout.device).contiguous()
        call("pmg_laplacian_set_coefficient_tensor", self._handle, ptr(t), current_stream())

    def has_coefficient_tensor(self) -> bool:
        return bool(call("pmg_laplacian_has_coefficient_tensor", self._handle))

    def set_reaction(self, sigma):
        """Per-cell reaction coefficient (``pmg_laplacian_set_reaction``): the operator becomes
        -div(K grad u) + sigma u, i.e. y = A x + d * x on unmarked rows with the lumped (GLL) mass vector d of sigma.
        ``sigma`` is a float64 numpy array (uploaded here) or torch tensor of shape ``(ncells,)``, one finite value
        >= 0 per local cell, ghost cells included; or ``None`` to remove the term.  The library keeps d, not sigma.  A
        computed inverse diagonal is rebuilt; not inside a stream capture."""
        self.coefficient_epoch += 1
        import torch

        if sigma is None:
            call("pmg_laplacian_set_reaction", self._handle, None, current_stream())
            return
        if not isinstance(sigma, (np.ndarray, torch.Tensor)):
            raise TypeError("set_reaction takes a float64 numpy array or torch tensor, or None")
        if sigma.dtype not in (np.float64, torch.float64):
            raise TypeError(f"the reaction coefficient must be float64, not {sigma.dtype}")
        if tuple(sigma.shape) != (self.ncells,):
            raise ValueError(f"the reaction coefficient has shape {tuple(sigma.shape)}, the operator needs "
                             f"({self.ncells},)")
        if isinstance(sigma, np.ndarray):
            sigma = torch.from_numpy(np.ascontiguousarray(sigma))
        sigma = sigma.to(self.layout.device).contiguous()
        call("pmg_laplacian_set_reaction", self._handle, ptr(sigma), current_stream())

    def has_reaction(self) -> bool:
        return bool(call("pmg_laplacian_has_reaction", self._handle))

    def geometry(self):
        """G in the reference layout [ncells, nq, 6] (device tensor), as the kernels read it (with the
        coefficient field and the coefficient tensor, if set)."""
        import torch

        N = (self.degree + 1) ** 3
        out = torch.empty((self.ncells, N, 6), dtype=torch.float64, device=self.layout.device)
        call("pmg_laplacian_get_geometry", self._handle, ptr(out), current_stream())
        return out

    def assemble_rhs(self, f: Vector, b: Vector):
        call("pmg_laplacian_assemble_rhs", self._handle, ptr(f.data), ptr(b.data), current_stream())

    def _boundary_vectors(self, what, g, b, x0):
        n = self.layout.size_local + self.layout.num_ghosts
        for name, v in (("g", g), ("b", b)) + ((("x0", x0),) if x0 is not None else ()):
            if not isinstance(v, Vector):
                raise TypeError(f"{what}: {name} must be a Vector of the operator's layout")
            if v.data.numel() != n:
                raise ValueError(f"{what}: {name} has {v.data.numel()} entries, the operator's layout {n}")

    def apply_lifting(self, g: Vector, b: Vector, x0: Vector = None, alpha: float = 1.0):
        """dolfinx ``fem.apply_lifting`` for this operator (``pmg_laplacian_apply_lifting``):
        b[i] -= alpha * sum_{j marked} A_ij (g[j] - x0[j]) on the owned unmarked rows, A without row / column
        treatment.  Unmarked entries of ``g`` / ``x0`` are never read; the ghosts of ``g`` are refreshed."""
        self._boundary_vectors("apply_lifting", g, b, x0)
        call("pmg_laplacian_apply_lifting", self._handle, ptr(g.data), ptr(x0.data) if x0 is not None else None,
             float(alpha), ptr(b.data), current_stream())

    def set_bc(self, g: Vector, b: Vector, x0: Vector = None, alpha: float = 1.0):
        """dolfinx ``fem.set_bc``: b[i] = alpha * (g[i] - x0[i]) on the marked owned entries."""
        self._boundary_vectors("set_bc", g, b, x0)
        call("pmg_laplacian_set_bc", self._handle, ptr(g.data), ptr(x0.data) if x0 is not None else None,
             float(alpha), ptr(b.data), current_stream())

    def assemble_neumann(self, cells, local_facets, h, b: Vector):
        """b += GLL-collocated int h v ds over the listed facets (``pmg_laplacian_assemble_neumann``).  ``cells``
        (int32) and ``local_facets`` (int8, 2 * axis + side) are host arrays, e.g. ``BoxPartition.exterior_facets()``;
        ``h`` [nfacets, nd*nd] holds one value per facet point in the order of ``facet_nodes`` (numpy, uploaded here,
        or a float64 device tensor).  Marked rows are skipped."""
        import torch

        cells = np.ascontiguousarray(cells, dtype=np.int32)
        local_facets = np.ascontiguousarray(local_facets, dtype=np.int8)
        if cells.ndim != 1 or cells.shape != local_facets.shape:
            raise ValueError("assemble_neumann: cells and local_facets are two lists of one length")
        nf = (self.degree + 1) ** 2
        if isinstance(h, torch.Tensor):
            if h.dtype != torch.float64 or not h.is_contiguous():
                raise TypeError("assemble_neumann: h must be a contiguous float64 tensor")
        else:
            h = _dev_f64(np.asarray(h, dtype=np.float64).reshape(-1), self.layout.device)
        if h.numel() != cells.size * nf:
            raise ValueError(f"assemble_neumann: h has {h.numel()} entries, {cells.size} facets need {cells.size * nf}")
        self._boundary_vectors("assemble_neumann", b, b, None)
        call("pmg_laplacian_assemble_neumann", self._handle, int(cells.size), cells.ctypes.data_as(_lib.c_ip),
             local_facets.ctypes.data_as(_lib.c_bp), ptr(h), ptr(b.data), current_stream())

    def set_robin(self, cells, local_facets, alpha):
        """Robin boundary term K grad u . n + alpha u = g on the listed facets (``pmg_laplacian_set_robin``): the
        operator gains the diagonal face mass d_R[dof] = sum of w1[i] w1[j] |dS| alpha over the facet points on the
        dof, beside the reaction term's vector; marked rows stay y = x.  ``cells`` (int32) and ``local_facets`` (int8,
        2 * axis + side) are host arrays as in ``assemble_neumann``, e.g. ``BoxPartition.exterior_facets()``;
        ``alpha`` [nfacets, nd*nd] holds one finite value >= 0 per facet point in the order of ``facet_nodes`` (numpy,
        uploaded here, or a float64 device tensor).  ``cells`` of length 0 or ``alpha=None`` removes the term.  The
        data g enters the right-hand side through ``assemble_neumann`` with ``h = g``.  A computed inverse diagonal is
        rebuilt; collective on several ranks; not inside a stream capture."""
        self.coefficient_epoch += 1
        import torch

        cells = np.ascontiguousarray(cells if cells is not None else [], dtype=np.int32)
        if alpha is None or cells.size == 0:
            call("pmg_laplacian_set_robin", self._handle, 0, None, None, None, current_stream())
            return
        local_facets = np.ascontiguousarray(local_facets, dtype=np.int8)
        if cells.ndim != 1 or cells.shape != local_facets.shape:
            raise ValueError("set_robin: cells and local_facets are two lists of one length")
        nf = (self.degree + 1) ** 2
        if isinstance(alpha, torch.Tensor):
            if alpha.dtype != torch.float64 or not alpha.is_contiguous():
                raise TypeError("set_robin: alpha must be a contiguous float64 tensor")
        else:
            alpha = _dev_f64(np.asarray(alpha, dtype=np.float64).reshape(-1), self.layout.device)
        if alpha.numel() != cells.size * nf:
            raise ValueError(f"set_robin: alpha has {alpha.numel()} entries, {cells.size} facets need "
                             f"{cells.size * nf}")
        call("pmg_laplacian_set_robin", self._handle, int(cells.size), cells.ctypes.data_as(_lib.c_ip),
             local_facets.ctypes.data_as(_lib.c_bp), ptr(alpha), current_stream())

    def has_robin(self) -> bool:
        return bool(call("pmg_laplacian_has_robin", self._handle))

    CELL_FORM_KAPPA = 1  # PMG_CELL_FORM_KAPPA
    CELL_FORM_CONSTRAINED = 2  # PMG_CELL_FORM_CONSTRAINED

    def cell_form(self, u, v, out=None, kappa: bool = True, constrained: bool = False):
        """The diffusion term's bilinear form cell by cell (``pmg_laplacian_cell_form``):
        e_c(u, v) = sum_q (grad_ref v)_q^T G_q (grad_ref u)_q, times ``kappa[c]`` (read now) with ``kappa=True``; with
        ``constrained=True`` the marked dofs of ``u`` and ``v`` read as zero.  ``u`` and ``v`` are ``Vector``s or
        contiguous float64 device tensors of the layout's total size and may be the same object; their ghost entries
        must be current: the call does not exchange.  Returns ``out``, a float64 device tensor ``[ncells]`` (made
        here when ``None``) with one value per cell of the dofmap, ghost cells included.  One launch; capturable.
        The reaction and Robin terms are not part of the form."""
        import torch

        n = self.layout.size_local + self.layout.num_ghosts
        args = []
        for name, t in (("u", u), ("v", v)):
            if isinstance(t, Vector):
                t = t.data
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError(f"{name} must be a Vector or a contiguous float64 torch tensor")
            if t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, the layout {n}")
            args.append(t)
        if out is None:
            out = torch.empty(self.ncells, dtype=torch.float64, device=self.layout.device)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_contiguous():
                raise TypeError("out must be a contiguous float64 torch tensor")
            if out.numel() != self.ncells:
                raise ValueError(f"out has {out.numel()} entries, the operator {self.ncells} cells")
        flags = (self.CELL_FORM_KAPPA if kappa else 0) | (self.CELL_FORM_CONSTRAINED if constrained else 0)
        call("pmg_laplacian_cell_form", self._handle, vp(args[0].data_ptr()), vp(args[1].data_ptr()),
             vp(out.data_ptr()), flags, current_stream())
        return out

    GRADIENTS = ("kappa", "field", "tensor", "sigma")  # the outputs of pmg_laplacian_form_gradients, in its order

    def form_gradients(self, u, v, kappa: bool = False, field: bool = False, tensor: bool = False,
                       sigma: bool = False, constrained: bool = True, out=None):
        """The derivatives of ``v_m^T A u_m`` with respect to the coefficients (``pmg_laplacian_form_gradients``), for
        the names requested: ``kappa`` [ncells], ``field`` [size_local + num_ghosts] (the nodal coefficient),
        ``tensor`` [ncells, 6] and ``sigma`` [ncells] (the reaction coefficient).  Each coefficient's own value is
        divided out, the others stay in as currently set; a gradient exists whether or not its coefficient is set.
        With ``constrained=True`` the marked dofs of ``u`` and ``v`` read as zero.  ``u`` and ``v`` are as in
        ``cell_form``: no exchange.  ``out`` may hold contiguous float64 device tensors for some of the requested
        names; the others are made here.  Returns a dict name -> tensor.  One fill (with ``field``) and one launch;
        capturable."""
        import torch

        n = self.layout.size_local + self.layout.num_ghosts
        args = []
        for name, t in (("u", u), ("v", v)):
            if isinstance(t, Vector):
                t = t.data
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError(f"{name} must be a Vector or a contiguous float64 torch tensor")
            if t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, the layout {n}")
            args.append(t)
        shapes = {"kappa": (self.ncells,), "field": (n,), "tensor": (self.ncells, 6), "sigma": (self.ncells,)}
        wanted = dict(zip(self.GRADIENTS, (kappa, field, tensor, sigma)))
        if not any(wanted.values()):
            raise ValueError("form_gradients: no gradient requested")
        out = dict(out) if out is not None else {}
        if set(out) - {k for k in self.GRADIENTS if wanted[k]}:
            raise ValueError(f"out names {sorted(set(out) - {k for k in self.GRADIENTS if wanted[k]})}, which "
                             "are not requested")
        res = {}
        for name in self.GRADIENTS:
            if not wanted[name]:
                continue
            t = out.get(name)
            if t is None:
                t = torch.empty(shapes[name], dtype=torch.float64, device=self.layout.device)
            elif not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError(f"out[{name!r}] must be a contiguous float64 torch tensor")
            elif t.numel() != int(np.prod(shapes[name])):
                raise ValueError(f"out[{name!r}] has {t.numel()} entries, the gradient {int(np.prod(shapes[name]))}")
            res[name] = t
        ptrs = [vp(res[k].data_ptr()) if k in res else None for k in self.GRADIENTS]
        call("pmg_laplacian_form_gradients", self._handle, vp(args[0].data_ptr()), vp(args[1].data_ptr()), *ptrs,
             self.CELL_FORM_CONSTRAINED if constrained else 0, current_stream())
        return res

    def lift_cell_count(self) -> int:
        """Cells that hold a marked dof (the lifting's work list); -1 before the first ``apply_lifting``."""
        return int(_lib.lib().pmg_laplacian_lift_cell_count(self._handle))

    def is_affine(self) -> bool:
        """Every cell is a parallelepiped (constant Jacobian)."""
        return bool(call("pmg_laplacian_is_affine", self._handle))

    def set_geometry_mode(self, mode: str):
        """"stored" (default, the reference's G[cell][q][6] stream) or "affine"
        (one constant tensor per cell; needs ``is_affine()``)."""
        call("pmg_laplacian_set_geometry_mode", self._handle, {"stored": 0, "affine": 1}[mode])

    def set_tensor_recompute(self, mode):
        """Recomputed tensor of a trilinear operator of degree 1 or 2 (include/pmg_amd.h): ``None`` / -1 automatic,
        ``False`` / 0 always stream G, ``True`` / 1 recompute it in the kernel (``PmgError`` on an operator that
        cannot)."""
        call("pmg_laplacian_set_tensor_recompute", self._handle, -1 if mode is None else int(mode))

    def tensor_recomputed(self) -> bool:
        """Does the next application form G in the kernel instead of streaming it?"""
        return bool(call("pmg_laplacian_tensor_recomputed", self._handle))

    def set_tensor_recompute_identity(self, mode):
        """The same switch for the degree-4 form, whose kernels take their transposes by identity
        (``pmg_laplacian_set_tensor_recompute_identity``): ``None`` / -1 automatic, ``False`` / 0, ``True`` / 1."""
        call("pmg_laplacian_set_tensor_recompute_identity", self._handle, -1 if mode is None else int(mode))

    def tensor_recomputed_identity(self) -> bool:
        """Does the next application of this degree-4 operator form G in the kernel?"""
        return bool(call("pmg_laplacian_tensor_recomputed_identity", self._handle))

    def set_column_tensor(self, mode):
        """The column-constant branch of the recomputed form (``pmg_laplacian_set_column_tensor``): items whose
        Jacobian does not change down their columns form the tensor once instead of once per layer.  ``None`` / -1
        automatic (on), ``False`` / 0, ``True`` / 1 (``PmgError`` on an operator whose apply does not recompute)."""
        call("pmg_laplacian_set_column_tensor", self._handle, -1 if mode is None else int(mode))

    def column_tensor(self) -> bool:
        """Does the next application run the kernels with the column-constant branch?"""
        return bool(call("pmg_laplacian_column_tensor", self._handle))

    def column_tensor_items(self):
        """(qualifying, total): the operator's work items that take the branch, counted with the kernels' own test."""
        import ctypes

        q, n = ctypes.c_longlong(0), ctypes.c_longlong(0)
        call("pmg_laplacian_column_tensor_items", self._handle, ctypes.byref(q), ctypes.byref(n), None)
        return int(q.value), int(n.value)

    def launches_per_apply(self) -> int:
        return call("pmg_laplacian_launches_per_apply", self._handle)

    def apply_streams(self) -> int:
        """2 if the interior colour launches run as two halves on two streams (include/pmg_amd.h), else 1."""
        return call("pmg_laplacian_apply_streams", self._handle)

    def chain_available(self) -> bool:
        """Has the operator chains of patches (include/pmg_amd.h, "Chain form")?"""
        return bool(call("pmg_laplacian_chain_available", self._handle))

    def chain_form(self) -> bool:
        return bool(call("pmg_laplacian_chain_form", self._handle))

    def set_chain_form(self, on: bool):
        call("pmg_laplacian_set_chain_form", self._handle, 1 if on else 0)

    def time_kernel(self, x: Vector, y: Vector, reps: int) -> float:
        """Mean milliseconds of one stiffness-kernel launch (one patch colour);
        an operator application issues ``launches_per_apply()`` of them (HIP
        events on the launch stream)."""
        out = C.c_double()
        call("pmg_laplacian_time_kernel", self._handle, ptr(x.data), ptr(y.data), int(reps), C.byref(out),
             current_stream())
        return out.value

    def set_profiling(self, flag: bool):
        """Bracket the stiffness launches of every application with HIP events (in-situ timing)."""
        call("pmg_laplacian_set_profiling", self._handle, 1 if flag else 0)

    def read_profile(self):
        """(summed milliseconds, number of stiffness launches) recorded since the last read."""
        ms, n = C.c_double(), C.c_longlong()
        call("pmg_laplacian_read_profile", self._handle, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _lib.lib().pmg_laplacian_destroy(self._handle)
                self._handle = None
        except Exception:
            pass
