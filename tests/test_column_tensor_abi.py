"""The entry points of the column-constant tensor (include/pmg_amd.h): pmg_laplacian_set_column_tensor and its values
and refusals, pmg_laplacian_column_tensor, pmg_laplacian_column_tensor_items, the environment switch, and the switch's
place in what a captured graph is keyed by.

The graph test needs a result that tells the two settings apart, which their values (equal to rounding) do not on a
mesh whose sums arrive in any order.  On a column of 1 x 1 x 16 cells every dof has at most two addends, a cycle
repeats itself bit for bit (tests/test_gpu_chebyshev_recompute.py), and the two settings differ in the last bits: a
replay must reproduce the eager cycle of the setting it was asked for, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

NAMES = ("pmg_laplacian_set_column_tensor", "pmg_laplacian_column_tensor", "pmg_laplacian_column_tensor_items")


def test_header_binding_and_export_agree(built):
    """(tests/test_abi.py checks all declared symbols; this names the three.)  NULL: -1 / an error, without a device."""
    from pmg_dolfinx_amd import _lib

    header = open(os.path.join(os.path.dirname(HERE), "include", "pmg_amd.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.exported_symbols() and f"int {name}(pmg_laplacian op" in header and hasattr(L, name)
    assert L.pmg_laplacian_column_tensor(ctypes.c_void_p(0)) == -1
    for mode in (-1, 0, 1):
        assert L.pmg_laplacian_set_column_tensor(ctypes.c_void_p(0), mode) != 0
    q, n = ctypes.c_longlong(0), ctypes.c_longlong(0)
    assert L.pmg_laplacian_column_tensor_items(ctypes.c_void_p(0), ctypes.byref(q), ctypes.byref(n), None) != 0


@pytest.fixture(scope="module")
def pm(built):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _op(pm, P, n=(2, 2, 8), **kw):
    from test_gpu_tensor_recompute import _operator

    part = pm.BoxPartition(n, **kw)
    return (part,) + _operator(pm, part, P, part.level(P).bc_marker)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 4])
def test_values_of_the_setter(pm, P):
    from pmg_dolfinx_amd import _lib

    part, lv, layout, op = _op(pm, P)
    assert op.column_tensor()  # automatic: on
    for mode, want in ((False, False), (True, True), (0, False), (1, True), (-1, True), (None, True)):
        op.set_column_tensor(mode)
        assert op.column_tensor() == want
    for bad in (-2, 2, 7):
        with pytest.raises(_lib.PmgError, match="pmg_laplacian_set_column_tensor: bad argument"):
            op.set_column_tensor(bad)
        assert op.column_tensor()
    q, total = op.column_tensor_items()
    assert q == total > 0  # a box
    # the switch follows the form it is a branch of: off the form there is nothing to switch, and mode 1 says so
    form = (lambda m: op.set_tensor_recompute_identity(m)) if P == 4 else (lambda m: op.set_tensor_recompute(m))
    form(False)
    assert not op.column_tensor()
    with pytest.raises(_lib.PmgError, match="does not recompute its tensor"):
        op.set_column_tensor(True)
    op.set_column_tensor(False)  # (0 and -1 are requests, never refused)
    op.set_column_tensor(None)
    assert not op.column_tensor()
    form(True)
    assert op.column_tensor()  # by itself: the request stands
    op.set_column_tensor(False)
    form(False)
    form(True)
    assert not op.column_tensor()


@pytest.mark.gpu
def test_refused_where_there_is_no_form(pm):
    """Degrees 3 and 5 have no recomputed form, a curved operator neither, and degree 1 has the form without the branch
    (column_branch, stiffness_column.hpp): mode 1 is refused, the report is 0, and the count has nothing to count."""
    from pmg_dolfinx_amd import _lib
    from test_gpu_fused_restriction import warp
    from test_gpu_tensor_recompute import _operator

    ops = [_op(pm, 3)[3], _op(pm, 5)[3]]
    part = pm.BoxPartition((3, 3, 4), warp=warp, geom_degree=2)
    ops.append(_operator(pm, part, 4, part.level(4).bc_marker, geometry_degree=2)[2])
    p1 = _op(pm, 1)[3]
    assert p1.tensor_recomputed()
    for op in ops + [p1]:
        assert not op.column_tensor()
        with pytest.raises(_lib.PmgError, match="has no column-constant branch" if op is p1 else
                           "does not recompute its tensor"):
            op.set_column_tensor(True)
        for mode in (False, None):
            op.set_column_tensor(mode)
            assert not op.column_tensor()
        with pytest.raises(_lib.PmgError, match="pmg_laplacian_column_tensor_items"):
            op.column_tensor_items()


@pytest.mark.gpu
def test_environment_switch(pm, monkeypatch):
    monkeypatch.setenv("PMG_COLUMN_TENSOR", "0")
    for P in (1, 2, 4):
        op = _op(pm, P)[3]
        assert not op.column_tensor() and (op.tensor_recomputed() or op.tensor_recomputed_identity())
    assert not _op(pm, 3)[3].column_tensor()
    monkeypatch.setenv("PMG_COLUMN_TENSOR", "1")
    for P in (2, 4):
        assert _op(pm, P)[3].column_tensor()
    assert not _op(pm, 3)[3].column_tensor() and not _op(pm, 1)[3].column_tensor()  # (no error: nothing to switch)
    monkeypatch.delenv("PMG_COLUMN_TENSOR")
    assert _op(pm, 4)[3].column_tensor()


@pytest.mark.gpu
def test_a_replayed_graph_follows_the_switch(pm):
    from test_gpu_column_tensor import COLUMN, warp_of
    from test_gpu_tensor_recompute import _cycles

    # (Dirichlet dofs on the face x = 0 only, so that the degree-1 level keeps free dofs: the column of
    # tests/test_gpu_chebyshev_recompute.py)
    h = pm.PoissonHierarchy(COLUMN, (1, 2, 4), kappa=2.0, cheb_its=3, warp=warp_of("extruded", COLUMN),
                            dirichlet=lambda c: c[:, 0] < 1e-12)

    def switch(on):
        for op in h.operators[1:]:  # (degrees 2 and 4: degree 1 has no branch)
            op.set_column_tensor(on)

    h.mg.set_graph(False)
    eager = {}
    for on in (True, False, True):
        switch(on)
        got = _cycles(h, 2)
        assert on not in eager or all(np.array_equal(a, b) for a, b in zip(got, eager[on]))  # reproducible here
        eager[on] = got
    assert not np.array_equal(eager[True][-1], eager[False][-1])  # the two settings can be told apart
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    for i, on in enumerate((True, False, False, True)):
        switch(on)
        got = _cycles(h, 2)
        assert h.mg.graph_replays() == n0 + 2 * (i + 1)
        assert all(np.array_equal(a, b) for a, b in zip(got, eager[on])), (i, on)
    h.mg.set_graph(False)
