"""What follows a change of the operator's data: the nodal field, the per-cell tensor, the reaction term and the Robin
term, set and removed on one operator in several orders.  Every setter goes through one rebuild function
(``laplacian_data_changed``); a rebuild it misses shows here as a stale tensor, float tensor, diagonal term or inverse
diagonal.

Meshes: 3 x 2 x 2 cells whose coordinate nodes are all moved by a seeded jitter, so no cell is affine.  P = 2 has the
flat, padded layout of the stored tensor and P = 3 the default one; a third case has P = 3 on a coordinate element of
degree 2 with the library's own tabulation.  The cells are handed over as two lists, so the operator holds more than
one patch and a batch can be smaller than the mesh.  The Dirichlet marker is the face x = 0, the Robin term sits on
the face x = 1.

The CPU truth is tests/curved_geometry_reference.py (it restates every quantity from J for any degree of the
coordinate element, g = 1 included) under tests/robin_reference.py's operator with the two diagonal vectors.  Bounds:
1e-12 relative for an FP64 apply and the inverse diagonal (tests/test_gpu_coefficient_tensor.py, test_gpu_reaction.py,
test_gpu_robin.py); 1e-5 for one FP32 apply (tests/test_gpu_mixed_precision.py); the exported tensor bit for bit
between operators that hold the same data -- every point is written by one thread, no atomics."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import curved_geometry_reference as cg  # noqa: E402
import robin_reference as rb  # noqa: E402
from tensor_coefficient_reference import random_spd  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12
TOL_FP32 = 1e-5
N = (3, 2, 2)
CASES = [(2, 1), (3, 1), (3, 2)]  # (P, degree of the coordinate element)
DATA = ("field", "tensor", "reaction", "robin")


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def jitter(x):
    """Every coordinate node moved by up to 0.02 (a sixth of the smallest node spacing at g = 2), seeded."""
    return x + np.random.default_rng(x.shape[0]).uniform(-0.02, 0.02, x.shape)


class Case:
    """The mesh, the four inputs and the oracle's operators, built once per (P, g) and never changed."""

    def __init__(self, pm, P, g):
        self.pm, self.P, self.g = pm, P, g
        self.part = pm.BoxPartition(N, warp=jitter, geom_degree=g)
        self.lv = lv = self.part.level(P)
        self.layout = pm.make_layout(lv)
        rng = np.random.default_rng(100 * P + g)
        straight = pm.BoxPartition(N, geom_degree=g).dof_coordinates(P)  # (the numbering does not depend on the map)
        self.bc = (lv.bc_marker.astype(bool) & (np.abs(straight[:, 0]) < 1e-12)).astype(np.int8)
        assert 0 < self.bc.sum() < lv.bc_marker.sum()
        nc = self.part.ncells
        self.kappa = rng.uniform(0.5, 1.5, nc) * 0.5 / P**2  # (test_gpu_robin.py: the terms are per cent of a row)
        self.kq = rng.uniform(0.5, 2.0, lv.ndofs)
        self.T = random_spd(nc, 7 * P + g)
        self.sigma = rng.uniform(0.0, 4.0, nc)
        cells, facets = self.part.exterior_facets()
        on = facets == 1  # the face x = 1
        self.cells, self.facets = cells[on], facets[on]
        assert self.cells.size == N[1] * N[2]
        self.alpha = rng.uniform(0.0, 4.0, (self.cells.size, (P + 1) ** 2))
        self.u = rng.standard_normal(lv.ndofs)
        self.lists = (np.arange(7, dtype=np.int32), np.arange(7, nc, dtype=np.int32))  # two cell lists: two patches

    def oracle(self, data=DATA):
        part, lv, P, g = self.part, self.lv, self.P, self.g
        A = cg.laplacian(P, g, self.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, self.bc)
        cg.with_tensor(A, self.T if "tensor" in data else None, self.kq if "field" in data else None)
        zero = np.zeros(lv.ndofs)
        d_sigma = cg.mass_vector(P, g, self.sigma, lv.dofmap, part.xgeom, part.geom_dofmap, self.bc) \
            if "reaction" in data else zero
        d_R = cg.facet_vector(P, g, lv.dofmap, part.xgeom, part.geom_dofmap, self.cells, self.facets, self.alpha,
                              self.bc) if "robin" in data else zero
        return rb.RobinLaplacian(A, d_R, d_sigma)

    def operator(self):
        pm, part, lv = self.pm, self.part, self.lv
        return pm.MatFreeLaplacian(self.P, self.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, self.lists[0],
                                   self.lists[1], self.bc, self.layout, geometry_degree=self.g)

    def vec(self, a):
        v = self.pm.Vector(self.layout)
        v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
        return v

    def set(self, op, what, on=True):
        if what == "field":
            op.set_coefficient_field(self.vec(self.kq) if on else None)
        elif what == "tensor":
            op.set_coefficient_tensor(self.T if on else None)
        elif what == "reaction":
            op.set_reaction(self.sigma if on else None)
        else:
            op.set_robin(self.cells, self.facets, self.alpha) if on else op.set_robin(None, None, None)

    def apply(self, op, u=None):
        """y = A u on the device; the marked rows must be y = u exactly."""
        u = self.u if u is None else u
        y = self.pm.Vector(self.layout)
        y.set(7.0)
        op(self.vec(u), y)
        got = y.data_copy()
        m = self.bc.astype(bool)
        assert np.array_equal(got[m], u[m])
        return got

    def apply_fp32(self, op, u):
        x = torch.from_numpy(u.astype(np.float32)).cuda()
        y = torch.full_like(x, 7.0)
        op.apply_fp32(x, y)
        torch.cuda.synchronize()
        return y.cpu().numpy().astype(np.float64)

    def diag(self, op):
        d = self.pm.Vector(self.layout)
        op.get_diag_inverse(d)
        return d.data_copy()


_CASES = {}


@pytest.fixture(params=CASES, ids=[f"P{P}-g{g}" for P, g in CASES])
def case(pm, request):
    if request.param not in _CASES:
        c = Case(pm, *request.param)
        c.full, c.plain = c.oracle(), c.oracle(())
        _CASES[request.param] = c
    return _CASES[request.param]


def _check(c, op, A, what):
    e_apply, e_diag = _relerr(c.apply(op), A.apply(c.u)), _relerr(c.diag(op), A.diag_inverse())
    print(f"P = {c.P}, g = {c.g}, {what}: apply {e_apply:.3e}, inverse diagonal {e_diag:.3e} (bound {TOL:.0e})")
    assert e_apply < TOL and e_diag < TOL


def test_order_does_not_matter(case):
    c = case
    first, second, fresh = c.operator(), c.operator(), c.operator()
    G0 = fresh.geometry()
    first.compute_diag_inverse()  # before the first set: every setter has to bring it up to date
    for what in DATA:
        c.set(first, what)
    for what in reversed(DATA):
        c.set(second, what)
    second.compute_diag_inverse()  # after the last
    G = first.geometry()
    assert torch.equal(G, second.geometry())
    assert not torch.equal(G, G0)
    _check(c, first, c.full, "set in order")
    _check(c, second, c.full, "set in reverse")
    assert _relerr(c.apply(first), c.apply(second)) < TOL and _relerr(c.diag(first), c.diag(second)) < TOL
    # (the four inputs are not small beside the operator: an oracle that lacks one is far away)
    for what in DATA:
        away = _relerr(c.oracle([d for d in DATA if d != what]).apply(c.u), c.full.apply(c.u))
        assert away > 1e-3, (what, away)
    # removed in a third order: the operator with nothing set
    for what in ("tensor", "robin", "field", "reaction"):
        c.set(first, what, on=False)
    assert torch.equal(first.geometry(), G0)
    _check(c, first, c.plain, "all four removed")


def test_batched_and_resident(case):
    from pmg_dolfinx_amd import _lib

    c = case
    resident, op = c.operator(), c.operator()
    for what in DATA:
        c.set(resident, what)
    G = resident.geometry()
    whole = _lib.lib().pmg_laplacian_geometry_bytes(op.handle)
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 1)  # one patch per batch (the Python class has no batching)
    assert 0 < _lib.lib().pmg_laplacian_geometry_bytes(op.handle) < whole
    op.compute_diag_inverse()
    for what in DATA:  # set while the tensor is not resident: every application recomputes it from the new data
        c.set(op, what)
    assert torch.equal(op.geometry(), G)
    _check(c, op, c.full, "batched geometry")
    _lib.call("pmg_laplacian_set_geometry_batch", op.handle, 0)
    assert _lib.lib().pmg_laplacian_geometry_bytes(op.handle) == whole
    assert torch.equal(op.geometry(), G)
    _check(c, op, c.full, "resident again")


def test_fp32_follows(case):
    c = case
    op = c.operator()
    u = c.u.astype(np.float32).astype(np.float64)
    c.apply_fp32(op, u)  # builds the float tensor: from here on every set has to rebuild it, or the float vector
    before = c.apply(op, u)
    for what in DATA:
        c.set(op, what)
        y64 = c.apply(op, u)
        err, moved = _relerr(c.apply_fp32(op, u), y64), _relerr(before, y64)
        print(f"P = {c.P}, g = {c.g}, after set {what}: FP32 against FP64 {err:.3e} (bound {TOL_FP32:.0e}); the set "
              f"moved the FP64 result by {moved:.3e}")
        assert moved > 1e3 * TOL_FP32  # (a float apply that missed this set would be that far away)
        assert err < TOL_FP32
        before = y64
