"""The distributed assembled operator without a GPU: the new entry points are declared in include/pmg_amd.h, exported by
the built library and bound, the header says what a distributed product does to its vectors, the old constructor's
contract is still stated, and the Python and C++ layers carry the feature."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("pmg_matrix_create_distributed", "pmg_matrix_cols", "pmg_matrix_export_split",
         "pmg_matrix_apply_ghosts_current")


def _header():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points():
    src, bare = _header()
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", bare))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_matrix_create_distributed\(pmg_matrix\* out, pmg_laplacian op, pmg_stream stream\);",
                     bare)
    assert re.search(r"long long\s+pmg_matrix_cols\(pmg_matrix M\);", bare)
    assert re.search(r"int\s+pmg_matrix_export_split\(pmg_matrix M, int32_t\* off_diag_offset, "
                     r"long long\* n_boundary_rows,\s*int32_t\* boundary_rows\);", bare)
    assert re.search(r"int\s+pmg_matrix_apply_ghosts_current\(pmg_matrix M, const double\* in, double\* out, "
                     r"pmg_stream stream\);", bare)
    # the product keeps its signature, and the header says what it does to the ghost entries
    assert re.search(r"int\s+pmg_matrix_apply\(pmg_matrix M, const double\* in, double\* out, pmg_stream stream\);",
                     bare)
    flat = re.sub(r"\s*\n\s*\*\s*", " ", src)
    assert re.search(r"REFRESHES THE GHOST ENTRIES OF `in`", flat)
    assert re.search(r"leaves the ghost entries of `out` alone", flat)
    # the single-domain constructor still states its refusal
    assert re.search(r"int\s+pmg_matrix_create_from_laplacian\(pmg_matrix\* out, pmg_laplacian op, pmg_stream stream\);",
                     bare)
    assert "single-domain only" in flat


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is an error with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_matrix_cols(None) == -1
    assert lib.pmg_matrix_create_distributed(None, None, None) == -1
    assert b"pmg_matrix_create_distributed" in lib.pmg_last_error()
    assert lib.pmg_matrix_export_split(None, None, None, None) == -1
    assert b"pmg_matrix_export_split" in lib.pmg_last_error()


def test_python_and_cpp_layers_carry_the_distributed_form(built):
    import pmg_dolfinx_amd as pm

    p = inspect.signature(pm.MatrixOperator.__init__).parameters
    assert list(p) == ["self", "laplacian", "distributed"] and p["distributed"].default is False
    assert callable(pm.MatrixOperator.export_split) and isinstance(pm.MatrixOperator.cols, property)
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "pmg_matrix_create_distributed(&_m" in hpp and "pmg_matrix_create_from_laplacian(&_m" in hpp
    assert "bool distributed() const" in hpp
    # the pattern and the split are host-only code a stand-alone program can include alone
    head = open(os.path.join(ROOT, "pmg-dolfinx_amd", "csrc", "matrix_pattern.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", head).lower()
    assert "matrix_pattern.hpp" in open(os.path.join(ROOT, "pmg-dolfinx_amd", "csrc", "matrix.hip")).read()
