"""Host mirror of ``acc::MatrixOperator`` (``src/csr.hpp:58-260``): the assembled CSR operator."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import call, current_stream, ptr, vp
from .laplacian import MatFreeLaplacian
from .vector import Vector


class MatrixOperator:
    """The BC-treated stiffness matrix of a :class:`MatFreeLaplacian`, assembled on the device
    (``MatrixOperator(a, bcs)``, ``:66-131``) and applied by SpMV.

    ``distributed=True`` builds the matrix on any layout, several ranks included (``pmg_matrix_create_distributed``):
    rows are the owned dofs, columns the local dofs with the ghosts last, and a product exchanges the halo of its
    input -- it refreshes the ghost entries of ``x`` and leaves those of ``y`` alone.  The default is the single-domain
    constructor, which refuses a layout with ghosts or a communicator.

    kappa is read when the values are assembled: after changing it in place call :meth:`update_values`.
    The matrix keeps its operator alive (it reads the operator's tensor, dofmap and markers)."""

    value_type = np.float64

    def __init__(self, laplacian: MatFreeLaplacian, distributed: bool = False):
        self.laplacian = laplacian
        self.layout = laplacian.layout
        self.distributed = bool(distributed)
        h = vp()
        call("pmg_matrix_create_distributed" if distributed else "pmg_matrix_create_from_laplacian", C.byref(h),
             laplacian.handle, current_stream())
        self._handle = h

    @property
    def handle(self):
        return self._handle

    def __call__(self, x: Vector, y: Vector):  # operator()(x, y), :220-260
        call("pmg_matrix_apply", self._handle, ptr(x.data), ptr(y.data), current_stream())

    def apply_ghosts_current(self, x: Vector, y: Vector):
        """``y = A x`` where the ghost entries of ``x`` are current already: no exchange, one launch."""
        call("pmg_matrix_apply_ghosts_current", self._handle, ptr(x.data), ptr(y.data), current_stream())

    def get_diag_inverse(self, diag_inv: Vector):  # :205-209
        call("pmg_matrix_get_diag_inverse", self._handle, ptr(diag_inv.data), current_stream())

    def update_values(self):
        """Re-assemble the values (and the inverse diagonal) on the existing pattern."""
        call("pmg_matrix_update_values", self._handle, current_stream())

    @property
    def nnz(self) -> int:  # :92-93
        return call("pmg_matrix_nnz", self._handle)

    @property
    def rows(self) -> int:
        return call("pmg_matrix_rows", self._handle)

    @property
    def cols(self) -> int:
        """Columns: the owned and the ghost dofs of the layout."""
        return call("pmg_matrix_cols", self._handle)

    @property
    def nbytes(self) -> int:
        """Device bytes held by the matrix."""
        return call("pmg_matrix_bytes", self._handle)

    def norm(self) -> float:
        """Frobenius norm of the stored values (the "A norm" of ``:95-99``), over all ranks (collective)."""
        out = C.c_double()
        call("pmg_matrix_frobenius_norm", self._handle, C.byref(out))
        return out.value

    def export(self):
        """(row_ptr, cols, values) as host arrays: this rank's rows, local column numbers."""
        n, nnz = self.rows, self.nnz
        rp = np.zeros(n + 1, dtype=np.int32)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        v = np.zeros(max(nnz, 1), dtype=np.float64)
        call("pmg_matrix_export", self._handle, None, None, rp.ctypes.data_as(_lib.c_ip), ci.ctypes.data_as(_lib.c_ip),
             v.ctypes.data_as(_lib.c_dp))
        return rp, ci[:nnz], v[:nnz]

    def export_split(self):
        """(off_diag_offset, boundary_rows) as host arrays: per row the position in ``cols`` of its first ghost column
        (``row_ptr[i + 1]`` where it has none), and the rows that have one, ascending."""
        n = self.rows
        nb = C.c_longlong()
        call("pmg_matrix_export_split", self._handle, None, C.byref(nb), None)
        od = np.zeros(max(n, 1), dtype=np.int32)
        br = np.zeros(max(nb.value, 1), dtype=np.int32)
        call("pmg_matrix_export_split", self._handle, od.ctypes.data_as(_lib.c_ip), None, br.ctypes.data_as(_lib.c_ip))
        return od[:n], br[:nb.value]

    def to_scipy(self):
        import scipy.sparse as sp

        rp, ci, v = self.export()
        return sp.csr_matrix((v, ci, rp), shape=(self.rows, self.cols))

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _lib.lib().pmg_matrix_destroy(self._handle)
                self._handle = None
        except Exception:
            pass
