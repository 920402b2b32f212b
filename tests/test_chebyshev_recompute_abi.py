"""The recomputed Chebyshev form without a GPU: its two entry points are declared, exported and bound, refuse bad
arguments with a message, the Python layer carries them, and the stored and the recomputed kernels share one definition
of the correction formula (the reason the two forms agree bit for bit, tests/test_gpu_chebyshev_recompute.py)."""
import ctypes as C
import inspect
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NAMES = ("pmg_chebyshev_set_recompute", "pmg_chebyshev_recomputed")


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "pmg_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmg_[a-z0-9_]+)\s*\(", bare))
    for name in NAMES:
        assert name in declared
    assert re.search(r"int\s+pmg_chebyshev_set_recompute\(pmg_chebyshev s, int mode\);", bare)
    assert re.search(r"long long\s+pmg_chebyshev_recomputed\(pmg_chebyshev s\);", bare)
    # the header says what the switch cannot change, and names the environment variable
    assert re.search(r"bit for bit", src) and "PMG_CHEB_RECOMPUTE" in src


def test_library_exports_and_binds_them(built):
    import pmg_dolfinx_amd as pm

    L = C.CDLL(pm._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in pmg_amd.h but not exported"
        assert name in pm._lib.exported_symbols()
    # host-only behaviour: a NULL handle is an error with a message, not a crash
    lib = pm._lib.lib()
    assert lib.pmg_chebyshev_recomputed(None) == -1
    assert lib.pmg_chebyshev_set_recompute(None, 1) == -1
    assert b"pmg_chebyshev_set_recompute" in lib.pmg_last_error()
    assert "pmg_chebyshev_recomputed" in pm._lib._COUNT_FUNCS
    assert pm._lib._SIGS["pmg_chebyshev_recomputed"][0] is C.c_longlong


def test_python_layer_carries_the_switch_and_the_count(built):
    import pmg_dolfinx_amd as pm

    for method in ("set_recompute", "recomputed"):
        assert callable(getattr(pm.Chebyshev, method))
    p = inspect.signature(pm.Chebyshev.set_recompute).parameters
    assert list(p) == ["self", "mode"] and p["mode"].default is None
    assert list(inspect.signature(pm.Chebyshev.recomputed).parameters) == ["self"]


def test_both_forms_share_the_correction_helpers():
    """The formula c1 z + c2 dinv r is written once, in a helper that fixes its own roundings; no functor spells it
    out again (the compiler would be free to contract each copy differently)."""
    src = open(os.path.join(ROOT, "pmg-dolfinx_amd", "csrc", "vector.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert len(re.findall(r"\bT cheb_correction\(", code)) == 1
    assert len(re.findall(r"\bT cheb_first_correction\(", code)) == 1
    body = code[code.index("T cheb_correction("):]
    body = body[: body.index("}")]
    assert "#pragma clang fp contract(off)" in body and "fma(c1, z, t)" in body
    # every step functor, stored or recomputed, goes through it: 2 (pair) + 1 (one) calls in ChebStepF and ChebFirstF,
    # 2 in ChebRecomputeF::entry
    assert len(re.findall(r"= cheb_correction\(", code)) == 8
    assert not re.search(r"c1 \* vz", code) and not re.search(r"c0 \* (vd|dinv)", code)
