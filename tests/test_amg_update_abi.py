"""The in-place renewal of an AMG hierarchy without a GPU: the two entry points are declared, exported and bound, the
Python and C++ layers and the driver carry them, a NULL handle is refused with a message, and the four coefficient
setters' comments point to the call."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pmg_amg_update_values", "pmg_amg_updates")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", bare))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_amg_update_values\(pmg_amg amg, pmg_stream stream\);", bare)
    assert re.search(r"long long\s+pmg_amg_updates\(pmg_amg amg\);", bare)
    # field, tensor, reaction, Robin: "the caller's to renew" now names the call
    assert len(re.findall(r"caller's\s+\*?\s*to renew \(the hierarchy\s+\*?\s*in place, with\s+\*?\s*pmg_amg_update_values\)",
                          src)) == 4


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    lib = pm._lib.lib()
    assert lib.pmg_amg_updates(None) == -1
    assert lib.pmg_amg_update_values(None, None) == -1
    assert b"pmg_amg_update_values" in lib.pmg_last_error()


def test_python_cpp_and_driver_carry_the_call(built):
    import pmg_dolfinx_amd as pm

    for method in ("update_values", "updates"):
        assert callable(getattr(pm.AmgSolver, method))
        assert list(inspect.signature(getattr(pm.AmgSolver, method)).parameters) == ["self"]
    hpp = open(os.path.join(ROOT, "include", "pmg_amd.hpp")).read()
    assert "void update_values() { check(pmg_amg_update_values(_a, nullptr)); }" in hpp
    src = open(os.path.join(ROOT, "examples", "pmg", "pmg_main.cpp")).read()
    assert '"--amg-renew"' in src and "update_values()" in src
    # created before the coefficient options, renewed after them
    assert src.index("o.amg_renew) // the hierarchy of the operator as created") < src.index("set_coefficient_field(")
    assert src.index("set_robin(") < src.index("coarse_solver->update_values()")
