"""pmg_amg_update_values: an AMG hierarchy renewed in place, on the device, after the operator's data changed.

The restatement.  The frozen aggregates are ``ao.aggregate(A_l, 0.08 / 2**l)`` on the hierarchy exported BEFORE the
update.  After it, per level, from the library's own exported A_l and rho_l:
  P_l      against ao.smoothed_prolongator(A_l, agg_l, na_l, rho_l)          <= 1e-13 max
  A_{l+1}  against P_l^T A_l P_l                                              <  1e-12 max
  A_0      against the oracle's assembled operator with the changed data      <  1e-12 max
  rho_l    against 1.05 ao.power_bound(A_l)                                   <= 1e-11 relative
the tolerances tests/test_gpu_amg_setup.py holds the host set-up to.  The device adds the power method's norms in
another order than numpy (a tree per block of 256 slots, then a tree over the blocks' partials); every test prints
the largest relative difference it meets.

Meshes: the table of tests/test_gpu_amg_setup.py -- "two-levels", "unwarped" (zeros in A_0 that depend on the
coefficient: the created P_0 is sparser than its structure), "row-blocks" (three levels), "kappa-jump" (rows outside the coarse space), "slab"
(lane width 2).  The Robin term lives on unmarked boundary dofs, so it has operators of its own with the marker on
x = 0 only."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import reaction_reference as rr  # noqa: E402
import robin_reference as rb  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402
from test_gpu_amg_setup import CASES as SETUP_CASES, twist  # noqa: E402

NAMES = ["two-levels", "unwarped", "row-blocks", "kappa-jump", "slab"]
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
_starts = {}


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def power_bound(A):
    from oracle import amg_oracle as ao

    n = A.shape[0]
    if n not in _starts:
        _starts[n] = ao.mt_uniform_half_one(n)
    return ao.power_bound(A, x0=_starts[n])


def exported(amg):
    L = amg.num_levels()
    return ([amg.export(l, "A") for l in range(L)], [amg.export(l, "P") for l in range(L - 1)],
            [amg.level_info(l)["lambda_max"] for l in range(L)])


def as_bytes(amg):
    As, Ps, rhos = exported(amg)
    return [a.tobytes() for M in As + Ps for a in (M.indptr, M.indices, M.data)] + [np.array(rhos).tobytes()]


class _Problem:
    """A degree-1 operator on one of the meshes, its hierarchy as created, and the frozen aggregates."""

    def __init__(self, pm, name, marker=None, **solver):
        from oracle import amg_oracle as ao

        n, warp, kappa, _ = SETUP_CASES[name]
        self.part = pm.BoxPartition(n, warp=warp)
        self.lv = self.part.level(1)
        self.layout = pm.make_layout(self.lv)
        self.kappa = kappa(self.lv.dofmap.shape[0]) if callable(kappa) else kappa
        self.marker = self.lv.bc_marker if marker is None else marker(self.lv.bc_marker, self.part.dof_coordinates(1))
        self.op = pm.MatFreeLaplacian(1, self.kappa, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap,
                                      self.lv.lcells, self.lv.bcells, self.marker, self.layout)
        self.op.compute_diag_inverse()
        self.pm, self.solver = pm, solver
        self.amg = pm.AmgSolver(self.op, **solver)
        self.As, self.Ps, self.rhos = exported(self.amg)
        self.aggs = [ao.aggregate(A, 0.08 / 2 ** l) for l, A in enumerate(self.As[:-1])]
        self.bc = self.marker.astype(bool)
        self.centres = tr.cell_centres(self.part.xgeom, self.part.geom_dofmap)
        self.coords = self.part.dof_coordinates(1)

    def oracle(self, T=None, kq=None):
        A = tr.laplacian(1, self.kappa, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap, self.marker)
        if T is not None or kq is not None:
            tr.with_tensor(A, np.tile(IDENTITY, (self.centres.shape[0], 1)) if T is None else T, kq)
        return A

    def field(self):  # the README's nodal field
        c = self.coords
        return 1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1]) + c[:, 2]

    def jump(self):  # 1 or 100 per cell, as an isotropic tensor
        s = np.where(np.random.default_rng(3).random(self.centres.shape[0]) < 0.5, 1.0, 100.0)
        return s[:, None] * IDENTITY[None, :]

    def update(self, amg=None):
        self.op.compute_diag_inverse()
        (self.amg if amg is None else amg).update_values()

    def restated_levels(self, A0):
        """The renewed hierarchy in numpy from the level-0 matrix A0: frozen aggregates, everything else anew."""
        from oracle import amg_oracle as ao

        As, Ps, rhos = [A0.tocsr()], [], []
        for agg, na in self.aggs:
            rhos.append(1.05 * power_bound(As[-1]))
            Ps.append(ao.smoothed_prolongator(As[-1], agg, na, rhos[-1]))
            As.append((Ps[-1].T @ (As[-1] @ Ps[-1])).tocsr())
        rhos.append(1.05 * power_bound(As[-1]))
        return As, Ps, rhos


def check_restatement(p, want0, what, amg=None):
    """The restatement of the module docstring on what ``amg`` exports now; returns the largest relative difference of
    a bound."""
    from oracle import amg_oracle as ao

    As, Ps, rhos = exported(p.amg if amg is None else amg)
    assert [A.shape[0] for A in As] == [A.shape[0] for A in p.As]
    e0 = abs(As[0] - want0).max() / abs(want0).max()
    worst = {"A0": e0, "rho": 0.0, "P": 0.0, "A": 0.0}
    for l, A in enumerate(As):
        want = 1.05 * power_bound(A)
        worst["rho"] = max(worst["rho"], abs(rhos[l] - want) / want)
    for l, (agg, na) in enumerate(p.aggs):
        want = ao.smoothed_prolongator(As[l], agg, na, rhos[l])
        worst["P"] = max(worst["P"], abs(Ps[l] - want).max() / abs(want).max())
        assert np.diff(Ps[l].indptr)[agg < 0].sum() == 0  # rows outside the coarse space stay empty
        Ac = (Ps[l].T @ (As[l] @ Ps[l])).tocsr()
        worst["A"] = max(worst["A"], abs(As[l + 1] - Ac).max() / abs(Ac).max())
    print(f"{what}: A_0 {worst['A0']:.2e}, bounds {worst['rho']:.2e}, P {worst['P']:.2e}, Galerkin {worst['A']:.2e}")
    assert worst["A0"] < 1e-12 and worst["rho"] <= 1e-11 and worst["P"] <= 1e-13 and worst["A"] < 1e-12
    return worst["rho"]


def check_against_created(p, scale, what):
    """Every A_l is ``scale`` times the created one, every P_l and rho_l the created one (tests/test_gpu_amg_setup.py's
    test_levels_equal_the_restated_build: 1e-12 max, 1e-10; P 1e-13 max)."""
    import scipy.sparse as sp

    As, Ps, rhos = exported(p.amg)
    assert [A.shape for A in As] == [A.shape for A in p.As]
    # (the identity rows of the marked dofs, which level 0 alone has, do not scale with the coefficient)
    want = [sp.diags(np.where(p.bc, 1.0, scale)) @ p.As[0]] + [scale * B for B in p.As[1:]]
    eA = max(abs(A - B).max() / abs(B).max() for A, B in zip(As, want))
    eP = max([abs(P - Q).max() / abs(Q).max() for P, Q in zip(Ps, p.Ps)] + [0.0])
    er = max(abs(r - q) / q for r, q in zip(rhos, p.rhos))
    print(f"{what}: against the created hierarchy: A {eA:.2e}, P {eP:.2e}, bounds {er:.2e}")
    assert eA < 1e-12 and eP <= 1e-13 and er <= 1e-10


# ---- 1, 2: unchanged data; kappa x 4 ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_unchanged_data_and_a_scaled_coefficient(pm, name):
    p = _Problem(pm, name)
    assert p.amg.updates() == 0
    p.amg.update_values()
    assert p.amg.updates() == 1
    check_against_created(p, 1.0, f"{name}, unchanged data")
    check_restatement(p, p.oracle().assemble_csr(), f"{name}, unchanged data")
    p.op.set_coefficient_tensor(np.tile(4.0 * IDENTITY, (p.centres.shape[0], 1)))
    p.update()
    assert p.amg.updates() == 2
    check_against_created(p, 4.0, f"{name}, K = 4 I")


# ---- 3: changed coefficients, each through its setter on the same operator ---------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_changed_coefficients_meet_the_restatement(pm, name):
    p = _Problem(pm, name)
    op = p.op
    T = tr.rotating_tensor(p.centres)
    op.set_coefficient_tensor(T)
    p.update()
    worst = check_restatement(p, p.oracle(T).assemble_csr(), f"{name}, rotating tensor")
    op.set_coefficient_tensor(p.jump())
    p.update()
    worst = max(worst, check_restatement(p, p.oracle(p.jump()).assemble_csr(), f"{name}, jump 1 / 100"))
    op.set_coefficient_tensor(None)
    op.set_coefficient_field(_vec(pm, p.layout, p.field()))
    p.update()
    worst = max(worst, check_restatement(p, p.oracle(kq=p.field()).assemble_csr(), f"{name}, nodal field"))
    op.set_coefficient_field(None)
    sigma = 3.0 * (1.0 + p.centres[:, 0])
    op.set_reaction(sigma)
    p.update()
    ref = rr.laplacian(1, p.kappa, sigma, p.lv.dofmap, p.part.xgeom, p.part.geom_dofmap, p.marker)
    worst = max(worst, check_restatement(p, ref.assemble_csr(), f"{name}, reaction"))
    op.set_reaction(None)
    p.update()
    check_against_created(p, 1.0, f"{name}, every term removed")
    assert p.amg.updates() == 5
    print(f"{name}: largest relative difference of a bound from numpy's: {worst:.2e}")


@pytest.mark.parametrize("name", ["two-levels", "slab"])
def test_robin_term_on_five_faces(pm, name):
    p = _Problem(pm, name, marker=rb.one_face_marker)
    cells, facets = p.part.exterior_facets()
    keep = facets != 0  # the face x = 0 keeps its Dirichlet marker
    cells, facets = cells[keep], facets[keep]
    alpha = rb.random_alpha(cells.size, 4, 5)
    p.op.set_robin(cells, facets, alpha)
    p.update()
    ref = rb.laplacian(p.part, 1, p.kappa, p.lv.dofmap, p.marker, cells, facets, alpha)
    assert ref.d_R.max() > 0
    check_restatement(p, ref.assemble_csr(), f"{name}, Robin term")
    p.op.set_robin(None, None, None)
    p.update()
    check_against_created(p, 1.0, f"{name}, Robin term removed")


# ---- 4: structure -------------------------------------------------------------------------------------------------
def test_structural_pattern_of_the_prolongator(pm):
    p = _Problem(pm, "unwarped")
    p.op.set_coefficient_tensor(tr.rotating_tensor(p.centres))
    p.update()
    P0, created = p.amg.export(0, "P"), p.Ps[0]
    mask = created.copy()
    mask.data[:] = 1.0
    outside = (P0 - P0.multiply(mask)).tocsr()
    outside.eliminate_zeros()
    print(f"unwarped: created P_0 {created.nnz} entries, renewed {P0.nnz}; {outside.nnz} outside the created pattern, "
          f"largest {abs(outside).max():.3e} of {abs(P0).max():.3e}")
    assert outside.nnz > 0 and abs(outside).max() > 1e-3 * abs(P0).max()
    assert (P0.data != 0.0).all()  # the structure holds nothing that this tensor leaves zero
    check_restatement(p, p.oracle(tr.rotating_tensor(p.centres)).assemble_csr(), "unwarped, rotating tensor")


def test_structural_counts_equal_the_created_ones_on_a_warped_mesh(pm):
    """On "two-levels" the structural and the created counts are equal, although the twisted 12^3 mesh has 8000 stored
    zeros among the 30657 entries of A_0: they are the body diagonals of the interior cells, which no quadrature point
    of the 2-point rule couples, so they are zero for every coefficient and do not count for the pattern of P_0
    (csrc/amg_renew.hpp, live_level0).  Every other entry of a warped cell's matrix is non-zero."""
    q = _Problem(pm, "two-levels")
    before = [q.amg.level_info(l)["nnz"] for l in range(2)]
    q.amg.update_values()
    after = [q.amg.level_info(l)["nnz"] for l in range(2)]
    print(f"two-levels: entries of A_l created {before}, structural {after}; P_0 created {q.Ps[0].nnz}, structural "
          f"{q.amg.export(0, 'P').nnz}")
    assert after == before
    assert q.amg.export(0, "P").nnz == q.Ps[0].nnz


# ---- 5: determinism -----------------------------------------------------------------------------------------------
def test_two_updates_from_the_same_data_give_the_same_bytes(pm):
    p = _Problem(pm, "row-blocks")
    p.op.set_coefficient_tensor(tr.rotating_tensor(p.centres))
    p.update()
    first = as_bytes(p.amg)
    p.amg.update_values()
    assert as_bytes(p.amg) == first


# ---- 6: solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-levels", "row-blocks"])
def test_krylov_solve_fresh_renewed_stale(pm, name):
    import scipy.sparse.linalg as spla

    from oracle.amg_oracle import AmgCycle

    p = _Problem(pm, name, max_iter=200, rtol=1e-8)
    stale = pm.AmgSolver(p.op, max_iter=200, rtol=1e-8)
    p.op.set_coefficient_tensor(p.jump())
    p.update()
    fresh = pm.AmgSolver(p.op, max_iter=200, rtol=1e-8)
    A = p.oracle(p.jump()).assemble_csr()
    b = np.random.default_rng(17).standard_normal(p.lv.ndofs)
    b[p.bc] = 0.0
    bv, x = _vec(pm, p.layout, b), pm.Vector(p.layout)
    its = {}
    for which, amg in (("renewed", p.amg), ("fresh", fresh), ("stale", stale)):
        its[which] = amg.solve(x, bv)
        if which == "renewed":
            got = x.data_copy()
    want = spla.spsolve(A.tocsc(), b)
    err = np.abs(got - want).max() / np.abs(want).max()
    _, its_ref = AmgCycle(*p.restated_levels(A), 2).pcg(lambda v: A @ v, b, 1e-8, 200)
    print(f"{name}, jump: iterations {its}, numpy on the restated renewed hierarchy {its_ref}; solution {err:.2e}")
    assert err <= 1e-6
    assert abs(its["renewed"] - its_ref) <= 1
    assert its["renewed"] <= its["fresh"] + 2
    assert its["stale"] >= 2 * its["renewed"]


# ---- 7: inside the V-cycle, graph replay on -----------------------------------------------------------------------
def test_renewal_inside_the_vcycle_with_graph_replay(pm):
    h = pm.PoissonHierarchy(8, (1, 2, 4), kappa=2.0, warp=twist)
    amg = pm.AmgSolver(h.operators[0], cycles=1)
    h.mg.set_coarse_solver(amg)
    h.mg.set_graph(True)
    x = h.new_vector()

    def apply():
        x.set(0.0)
        h.mg.apply(h.rhs[-1], x)
        torch.cuda.synchronize()
        return x.data_copy(), h.mg.apply_counts()

    before, _ = apply()
    replays = h.mg.graph_replays()
    assert replays == 1
    for P, op, layout in zip(h.orders, h.operators, h.layouts):
        c = h.part.dof_coordinates(P)
        op.set_coefficient_field(_vec(pm, layout, 1.0 + 0.5 * np.sin(2 * np.pi * c[:, 0]) * np.cos(2 * np.pi * c[:, 1])
                                      + c[:, 2]))
        op.compute_diag_inverse()
    amg.update_values()
    replayed, counts = apply()
    assert h.mg.graph_replays() == replays + 1
    h.mg.set_graph(False)
    eager, counts_eager = apply()
    err = np.abs(replayed - eager).max() / np.abs(eager).max()
    print(f"V-cycle after the renewal: graph against eager {err:.2e}; moved by the field "
          f"{np.abs(replayed - before).max() / np.abs(before).max():.2e}")
    assert err <= 1e-13 and counts == counts_eager
    assert np.abs(replayed - before).max() > 1e-3 * np.abs(before).max()


# ---- 8: null space ------------------------------------------------------------------------------------------------
def test_null_space_mode_follows_the_renewal(pm):
    part = pm.BoxPartition(10, warp=twist)
    lv = part.level(1)
    layout = pm.make_layout(lv)
    bc = np.zeros(lv.ndofs, dtype=np.int8)
    op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bc, layout)
    op.compute_diag_inverse()
    amg = pm.AmgSolver(op, max_iter=60, rtol=1e-8)
    assert amg.num_levels() == 2
    amg.set_nullspace("constant")
    b = np.random.default_rng(10).standard_normal(lv.ndofs)
    b -= b.mean()
    bv, x = _vec(pm, layout, b), pm.Vector(layout)
    amg.cycle(x, bv)
    first = x.data_copy()
    amg.update_values()
    amg.cycle(x, bv)
    again = x.data_copy()
    assert np.abs(again - first).max() <= 1e-12 * np.abs(first).max()
    assert abs(again.mean()) <= 1e-12 * np.abs(again).max()
    T = tr.rotating_tensor(tr.cell_centres(part.xgeom, part.geom_dofmap))
    op.set_coefficient_tensor(T)
    op.compute_diag_inverse()
    amg.update_values()
    its = amg.solve(x, bv)
    got = x.data_copy()
    A = tr.with_tensor(tr.laplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, bc), T).assemble_csr().toarray()
    want = np.linalg.lstsq(A, b, rcond=None)[0]
    want -= want.mean()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"pure Neumann, rotating tensor: {its} iterations, mean-free solution {err:.2e}")
    assert its < 60 and err <= 1e-6 and abs(got.mean()) <= 1e-12 * np.abs(got).max()


# ---- 9: refusals --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_hierarchy_alone(pm):
    from pmg_dolfinx_amd import _lib
    from pmg_dolfinx_amd._lib import current_stream

    p = _Problem(pm, "two-levels")
    N = p.lv.ndofs
    perm = np.random.default_rng(2024).permutation(N)
    replicated = pm.AmgSolver(p.op, global_index=perm, n_global=N)
    with pytest.raises(_lib.PmgError, match="replicated"):
        replicated.update_values()
    assert replicated.updates() == 0
    before = as_bytes(p.amg)
    side, scratch = torch.cuda.Stream(), torch.zeros(8, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc = _lib.lib().pmg_amg_update_values(p.amg.handle, current_stream())
            msg = _lib.lib().pmg_last_error()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert rc == -1 and b"pmg_amg_update_values" in msg and b"captured" in msg
    assert p.amg.updates() == 0 and as_bytes(p.amg) == before
    p.amg.update_values()  # ... and the call works afterwards
    assert p.amg.updates() == 1
