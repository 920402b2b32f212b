"""The constant null space without a GPU: pmg_vec_remove_mean, pmg_cg_set_nullspace / pmg_cg_nullspace and
pmg_amg_set_nullspace / pmg_amg_nullspace are declared, exported and bound, the Python layer carries them, and the
refusals that need no device -- a NULL handle, an unknown mode -- come back with their message."""
import ctypes as C
import inspect
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NAMES = ("pmg_vec_remove_mean", "pmg_cg_set_nullspace", "pmg_cg_nullspace", "pmg_amg_set_nullspace",
         "pmg_amg_nullspace")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", code))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_vec_remove_mean\(pmg_layout l, double\* x, const double\* w, pmg_stream \w+\);", code)
    assert re.search(r"int\s+pmg_cg_set_nullspace\(pmg_cg \w+, int mode\);", code)
    assert re.search(r"int\s+pmg_amg_set_nullspace\(pmg_amg \w+, int mode\);", code)
    assert re.search(r"#define\s+PMG_NULLSPACE_NONE\s+0\b", code)
    assert re.search(r"#define\s+PMG_NULLSPACE_CONSTANT\s+1\b", code)


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()


def test_null_handles_and_unknown_modes_are_refused_with_a_message(built):
    import pmg_dolfinx_amd as pm

    lib = pm._lib.lib()
    assert lib.pmg_vec_remove_mean(None, None, None, None) == -1
    assert b"pmg_vec_remove_mean" in lib.pmg_last_error()
    for name in ("pmg_cg", "pmg_amg"):
        setter, getter = getattr(lib, name + "_set_nullspace"), getattr(lib, name + "_nullspace")
        assert setter(None, 1) == -1
        assert (name + "_set_nullspace: NULL").encode() in lib.pmg_last_error()
        for mode in (2, -1, 7):
            assert setter(None, mode) == -1
            assert (name + f"_set_nullspace: unknown mode {mode}").encode() in lib.pmg_last_error()
        assert getter(None) == -1


def test_python_layer_carries_them(built):
    import pmg_dolfinx_amd as pm

    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(pm.Vector.remove_mean) == ["self", "weights"]
    assert inspect.signature(pm.Vector.remove_mean).parameters["weights"].default is None
    assert sig(pm.CGSolver.set_nullspace) == ["self", "mode"]
    assert sig(pm.AmgSolver.set_nullspace) == ["self", "mode"]
    assert pm._lib.nullspace_mode("constant") == 1 and pm._lib.nullspace_mode(None) == 0
    with pytest.raises(ValueError, match="unknown null space"):
        pm._lib.nullspace_mode("rigid-body")


def test_cpp_adapter_and_drivers_carry_them():
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert re.search(r"void remove_mean\(Vector& x\)", hpp)
    assert re.search(r"void remove_mean\(Vector& x, const Vector& w\)", hpp)
    assert len(re.findall(r"void set_nullspace\(bool constant\)", hpp)) == 2  # CGSolver and the AMG coarse solver
    for driver in ("pmg", "cg", "mat_free"):
        assert '"--neumann"' in open(os.path.join(ROOT, "examples", driver, driver + "_main.cpp")).read()
