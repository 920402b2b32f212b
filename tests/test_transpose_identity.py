"""The barycentric identity behind `transposes_by_identity` (pmg-dolfinx_amd/csrc/stiffness_column.hpp) and
`layer_backward_identity` (stiffness_layer.hpp), in numpy on the library's own 1-D derivative table (host entry point,
no GPU): for the Lagrange basis on distinct nodes

    (D^T f)_i = 2 D_ii f_i - rho_i sum_j D_ij (f_j / rho_j),        rho_i = -D_0i / D_i0  (rho_0 = 1),

with 2 D_ii picked out of row i, as the degree-4 kernels do beside the recomputed tensor, and 1 / rho_i formed as
-D_i0 / D_0i, as the fused kernel's table has it.

Bound: the two sides are sums of nd <= 9 products of table entries up to about nd^2 / 2 in size with |f| <= 1, one
division per rho and one per 1 / rho; rho spans up to about 1e2 between the end and the middle nodes, so a term carries
a few roundings of eps = 1.1e-16 on values up to about 1e2 * max |D| * max |f|.  1e-13 relative to max |D| * max |f|
* nd leaves a factor of a few above that and is eight orders below any wrong entry."""
import numpy as np
import pytest

from pmg_dolfinx_amd import _tables


@pytest.mark.parametrize("nd", [3, 5, 6, 9])
def test_transposed_contraction_by_identity(built, nd):
    D = _tables.lagrange_derivative_table(nd)
    rho = np.array([1.0] + [-D[0, i] / D[i, 0] for i in range(1, nd)])
    irho = np.array([1.0] + [-D[i, 0] / D[0, i] for i in range(1, nd)])
    assert np.all(rho > 0)  # (l_i / l_0)^2
    assert np.abs(rho * irho - 1.0).max() < 4e-16
    f = np.random.default_rng(nd).uniform(-1.0, 1.0, nd)
    want = D.T @ f
    got = 2.0 * np.diag(D) * f - rho * (D @ (f * irho))
    scale = np.abs(D).max() * nd
    err = np.abs(got - want).max() / scale
    print(f"nd = {nd}: identity against D^T f, {err:.3e} of max |D| * nd; rho in [{rho.min():.3g}, {rho.max():.3g}]")
    assert err < 1e-13


def test_every_pair_of_entries_obeys_the_identity(built):
    """D_ji = -(rho_i / rho_j) D_ij for i != j, entry by entry at nd = 5 (degree 4)."""
    nd = 5
    D = _tables.lagrange_derivative_table(nd)
    rho = np.array([1.0] + [-D[0, i] / D[i, 0] for i in range(1, nd)])
    for i in range(nd):
        for j in range(nd):
            if i != j:
                assert abs(D[j, i] * rho[j] + rho[i] * D[i, j]) < 1e-13 * np.abs(D).max() * rho.max()
