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
    (``MatrixOperator(a, bcs)``, ``:66-131``) and applied by SpMV.  Single domain only.

    kappa is read when the values are assembled: after changing it in place call :meth:`update_values`.
    The matrix keeps its operator alive (it reads the operator's tensor, dofmap and markers)."""

    value_type = np.float64

    def __init__(self, laplacian: MatFreeLaplacian):
        self.laplacian = laplacian
        self.layout = laplacian.layout
        h = vp()
        call("pmg_matrix_create_from_laplacian", C.byref(h), laplacian.handle, current_stream())
        self._handle = h

    @property
    def handle(self):
        return self._handle

    def __call__(self, x: Vector, y: Vector):  # operator()(x, y), :220-260
        call("pmg_matrix_apply", self._handle, ptr(x.data), ptr(y.data), current_stream())

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
    def nbytes(self) -> int:
        """Device bytes held by the matrix."""
        return call("pmg_matrix_bytes", self._handle)

    def norm(self) -> float:
        """Frobenius norm of the stored values (the "A norm" of ``:95-99``)."""
        out = C.c_double()
        call("pmg_matrix_frobenius_norm", self._handle, C.byref(out))
        return out.value

    def export(self):
        """(row_ptr, cols, values) as host arrays."""
        n, nnz = self.rows, self.nnz
        rp = np.zeros(n + 1, dtype=np.int32)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        v = np.zeros(max(nnz, 1), dtype=np.float64)
        call("pmg_matrix_export", self._handle, None, None, rp.ctypes.data_as(_lib.c_ip), ci.ctypes.data_as(_lib.c_ip),
             v.ctypes.data_as(_lib.c_dp))
        return rp, ci[:nnz], v[:nnz]

    def to_scipy(self):
        import scipy.sparse as sp

        rp, ci, v = self.export()
        return sp.csr_matrix((v, ci, rp), shape=(self.rows, self.rows))

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _lib.lib().pmg_matrix_destroy(self._handle)
                self._handle = None
        except Exception:
            pass
