"""The identity the fused apply-and-restrict kernel rests on (stiffness_restrict.hpp), on the numpy oracle alone:

    R (r - A z) = sum over cells  P_cell^T (r|cell / mult - A_cell z),

with the apply's Dirichlet rule (A z)_i = z_i on marked rows, i.e. a share of (r - z) / mult there and the cell's
product dropped.  It holds because P[f, c] is the same from every cell that holds the fine dof f and zero for every
coarse dof outside those cells.  No GPU."""
import numpy as np
import pytest

from oracle import pmg_oracle as po


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def cell_additive_restriction(A, I, z, r):
    """sum_cells P_cell^T (share - A_cell z): what one workgroup of the fused kernel adds up, cell by cell."""
    nd = A.nd
    bc = A.bc
    zm = np.where(bc, 0.0, z)  # Dirichlet columns masked, as in the apply
    Az = A.cell_apply(zm[A.dofmap].reshape(-1, nd, nd, nd)).reshape(A.ncells, -1)
    share = np.where(bc, r - z, r) / np.where(I.mult > 0, I.mult, 1.0)
    w = share[I.dmf] - np.where(bc[I.dmf], 0.0, Az)  # [ncells, Nf]
    return np.bincount(I.dmc.ravel(), weights=(w @ I.M).ravel(), minlength=I.nc)


@pytest.mark.parametrize("markers", [True, False])
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
@pytest.mark.parametrize("warped", [True, False])
@pytest.mark.parametrize("n", [(4, 4, 8), (5, 3, 7)])
def test_cell_additive_form_equals_restricted_residual(n, warped, pc, pf, markers):
    mesh = po.BoxMesh(n, warp=warp if warped else None)
    bcm = mesh.boundary_marker(pf) if markers else np.zeros(mesh.ndofs(pf), dtype=np.int8)
    kappa = 0.5 + np.random.default_rng(7).random(mesh.ncells)  # varies from cell to cell
    A = po.Laplacian(pf, kappa, mesh.dofmap(pf), mesh.xgeom, mesh.geom_dofmap, bcm)
    I = po.Interpolator(pc, pf, mesh.dofmap(pc), mesh.dofmap(pf), mesh.ndofs(pc), mesh.ndofs(pf))
    rng = np.random.default_rng(pc * 10 + pf)
    z, r = rng.standard_normal(A.ndofs), rng.standard_normal(A.ndofs)  # non-zero on the Dirichlet dofs as well
    if markers:
        assert np.abs(z[A.bc]).min() > 0.0
    ref = I.reverse_interpolate(r - A.apply(z))
    got = cell_additive_restriction(A, I, z, r)
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()
