"""The identity behind the column-constant branch of the recomputed tensor (TensorStream::column_constant, in
pmg-dolfinx_amd/csrc/stiffness_layer.hpp), in numpy alone.  Down the column (xi_a, eta_b) of a trilinear cell
J(zeta) = [jc0 + zeta jc1 | jc2 + zeta jc3 | jc4]; the slopes jc1, jc3 are built from the cell's zeta-cross
coefficients c101, c011, c111 alone.  So G(a, b, k) / w_k does not depend on k, for every column, if and only if the
three vanish: the top face of the cell is a translate of its bottom face.

Coordinates are multiples of 2^-6, so the coefficient differences are exact and a vanishing coefficient is an exact
zero, as on the meshes of tests/test_gpu_column_tensor.py.  Bounds: with exact zero slopes the column form gives the
same J in every layer, hence EQUAL tensors; the oracle's G (another order of operations, w_k multiplied in) agrees to
1e-13 of the tensor's largest entry (a few tens of roundings, the bound of tests/test_cell_frames.py).  Where a cross
coefficient of size 1/8 is present the dependence on k is of that order: it is asked to exceed 1e-3."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from oracle import pmg_oracle as po  # noqa: E402
from test_tensor_recompute_identity import cell_coefficients, column_pieces, column_tensor, twisted_cell  # noqa: E402

P = 4
REF = np.array([[i, j, l] for i in (0, 1) for j in (0, 1) for l in (0, 1)], dtype=np.float64)  # vertex 4 i + 2 j + l
C011, C101, C111 = 3, 5, 7  # rows of cell_coefficients: m = 4 i + 2 j + k


def box_cell():
    return REF * np.array([1.25, 0.75, 1.5]) + np.array([0.5, -0.25, 1.0])


def extruded_cell():
    """A general quadrilateral (no two sides parallel) in the plane z = 0.25, extruded along (0.15625, -0.125, 0.8125):
    a sheared extrusion direction."""
    quad = {(0, 0): (0.0, 0.0), (1, 0): (1.125, 0.09375), (0, 1): (-0.0625, 0.875), (1, 1): (1.3125, 1.0625)}
    v = np.empty((8, 3))
    for m, (i, j, l) in enumerate(REF.astype(int)):
        v[m] = np.array([*quad[(i, j)], 0.25]) + l * np.array([0.15625, -0.125, 0.8125])
    return v


def cross(v):
    """max |c101|, |c011|, |c111| of a cell"""
    return np.abs(cell_coefficients(v)[[C011, C101, C111]]).max()


def dependence(v):
    """The largest change of G(a, b, k) / w_k down a column, relative to the tensor's largest entry: by the column form
    (what the kernels evaluate) and by the oracle's G."""
    nd = P + 1
    pts, w = po.gll_points_weights(nd)
    dphi, w3 = po.geometry_tables(P)
    G, _ = po.geometry_G(v, np.arange(8, dtype=np.int32)[None, :], dphi, w3)
    c = cell_coefficients(v)
    form = oracle = agree = 0.0
    for a in range(nd):
        for b in range(nd):
            pieces = column_pieces(c, pts[a], pts[b], w[a] * w[b])
            col = np.array([column_tensor(pieces, pts[k], 1.0) for k in range(nd)])
            ora = np.array([G[0, (a * nd + b) * nd + k] / w[k] for k in range(nd)])
            size = np.abs(col).max()
            form = max(form, np.abs(col - col[0]).max() / size)
            oracle = max(oracle, np.abs(ora - ora[0]).max() / size)
            agree = max(agree, np.abs(col - ora).max() / size)
    assert agree < 1e-13  # (the column form is the oracle's tensor, whatever the cell)
    return form, oracle


@pytest.mark.parametrize("cell", [box_cell, extruded_cell])
def test_constant_down_every_column(cell):
    v = cell()
    assert cross(v) == 0.0
    form, oracle = dependence(v)
    print(f"{cell.__name__}: G / w_k down the columns moves by {form:.3e} (column form), {oracle:.3e} (oracle)")
    assert form == 0.0 and oracle < 1e-13


def test_extruded_cell_is_not_constant_across_columns():
    """What separates `constant down the column` from `constant in the cell` (the affine mode's class)."""
    v = extruded_cell()
    nd = P + 1
    pts, w = po.gll_points_weights(nd)
    c = cell_coefficients(v)
    g = np.array([column_tensor(column_pieces(c, pts[a], pts[b], 1.0), 0.0, 1.0) for a in range(nd) for b in range(nd)])
    assert np.abs(g - g[0]).max() / np.abs(g).max() > 1e-3


def test_general_cell_depends_on_the_layer():
    v = twisted_cell()
    assert cross(v) > 1e-2
    form, oracle = dependence(v)
    print(f"twisted cell: G / w_k down the columns moves by {form:.3e} (column form), {oracle:.3e} (oracle)")
    assert form > 1e-3 and oracle > 1e-3


@pytest.mark.parametrize("which", ["c101", "c011", "c111"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_each_cross_coefficient_alone_breaks_it(which, axis):
    """Only if: the extruded cell plus one zeta-cross monomial in one coordinate."""
    mono = {"c101": REF[:, 0] * REF[:, 2], "c011": REF[:, 1] * REF[:, 2], "c111": REF[:, 0] * REF[:, 1] * REF[:, 2]}
    v = extruded_cell()
    v[:, axis] += 0.125 * mono[which]
    c = cell_coefficients(v)
    row = {"c101": C101, "c011": C011, "c111": C111}[which]
    assert c[row, axis] == 0.125 and np.count_nonzero(c[[C011, C101, C111]]) == 1
    form, oracle = dependence(v)
    print(f"{which} in coordinate {axis}: {form:.3e} (column form), {oracle:.3e} (oracle)")
    assert form > 1e-3 and oracle > 1e-3


@pytest.fixture(scope="module")
def pm(built):
    import pmg_dolfinx_amd as pm

    return pm


def test_the_48_local_frames(pm):
    """The frames of tests/test_cell_frames.py on the extruded cell: the identity holds, exactly, in the 16 frames whose
    local zeta runs along the extrusion (old axis 2, either way round); in the other 32 the quadrilateral's own
    bilinear term has become a zeta-cross coefficient."""
    v = extruded_cell()
    holds = 0
    for perm, flips, _ in pm.cell_symmetries():
        new = v[pm.frame_node_map(1, perm, flips)]
        form, oracle = dependence(new)
        if perm[2] == 2:
            holds += 1
            assert cross(new) == 0.0 and form == 0.0 and oracle < 1e-13, (perm, flips)
        else:
            assert cross(new) > 1e-2 and form > 1e-3 and oracle > 1e-3, (perm, flips)
    assert holds == 16
