"""The constant null space on the device: pmg_vec_remove_mean, pmg_cg_set_nullspace, pmg_amg_set_nullspace on the pure
Neumann operator (an all-zero marker, no reaction, no Robin term).

The CPU truth is tests/nullspace_reference.py (pinned in tests/test_nullspace_reference.py) over the oracle's operator,
V-cycle and the AMG cycle on the hierarchy the library exports.

Bounds.  remove_mean: integer data must come out bit for bit (every summation order is exact, the mean is a quotient);
random data within n 2^-53 max|x|, the worst case of any summation order.  Mean of a solution: |1 . x| <= n 2^-53 max|x|.
Solutions follow the tolerance rule: with x_tight = pinv(A) b where the dense matrix is affordable (at most DENSE_MAX
dofs) and the restatement at rtol 1e-14 elsewhere, e_ref = |x_ref - x_tight| / |x_tight| for the restatement at the
test's rtol, the device result must satisfy |x_gpu - x_tight| / |x_tight| <= 10 e_ref + 1e-12.  Iteration counts are
within 1 of the restatement's.  NOISE = 1e-14 between two runs on the same bits; graph replay against eager 1e-12
(FP64) and 1e-6 (FP32 cycle); the device AMG cycle against the numpy cycle 1e-11 (tests/test_gpu_amg_setup.py's)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import boundary_data_reference as bd  # noqa: E402
import nullspace_reference as ns  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NOISE = 1e-14
EPS = 2.0 ** -53
DENSE_MAX = 800
MAPS = {None: None, "twist": bd.twist, "warp": bd.warp}


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data[: len(a)].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def _kappa(P, ncells, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, ncells) * 0.5 / P**2


def _rel2(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _mean_is_zero(x):
    return abs(x.sum()) <= x.size * EPS * np.abs(x).max()


def _nowhere(c):
    return c[:, 0] < -1.0


# ---- 1. remove_mean -----------------------------------------------------------------------------------------------


SIZES = [1, 2, 63, 64, 65, 257, 4 * 2**20 + 3]


@pytest.mark.parametrize("n", SIZES)
def test_remove_mean_integers_bit_for_bit(pm, n):
    x = np.random.default_rng(n).integers(-8, 9, n).astype(np.float64)
    layout = pm.Layout(n)
    v = _vec(pm, layout, x)
    v.remove_mean()
    assert np.array_equal(v.data_copy(), x - x.sum() / n)


@pytest.mark.parametrize("n", SIZES)
def test_remove_mean_random_plain_and_weighted(pm, n):
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal(n)
    w = rng.uniform(0.5, 1.5, n)
    layout = pm.Layout(n)
    bound = n * EPS * np.abs(x).max()
    v = _vec(pm, layout, x)
    v.remove_mean()
    plain = np.abs(v.data_copy() - ns.remove_mean(x)).max()
    v = _vec(pm, layout, x)
    v.remove_mean(_vec(pm, layout, w))
    weighted = np.abs(v.data_copy() - ns.remove_mean(x, w)).max()
    print(f"n = {n}: plain {plain:.3e}, weighted {weighted:.3e}, bound {bound:.3e}")
    assert plain <= bound
    assert weighted <= bound


def test_remove_mean_misaligned(pm):
    """x eight bytes off a 16-byte boundary: the scalar kernels."""
    from pmg_dolfinx_amd import _lib

    n = 257
    x = np.random.default_rng(3).integers(-8, 9, n).astype(np.float64)
    layout = pm.Layout(n)
    t = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
    off = 1 if t.data_ptr() % 16 == 0 else 2
    assert (t.data_ptr() + 8 * off) % 16 == 8
    t[off: off + n].copy_(torch.from_numpy(x))
    _lib.call("pmg_vec_remove_mean", layout.handle, _lib.vp(t.data_ptr() + 8 * off), _lib.vp(0), _lib.current_stream())
    got = t.cpu().numpy()
    assert np.array_equal(got[off: off + n], x - x.sum() / n)
    assert np.all(got[:off] == 0) and np.all(got[off + n:] == 0)


def test_remove_mean_shifts_the_ghosts_and_sums_the_owned(pm):
    n, g = 300, 37
    rng = np.random.default_rng(4)
    x = rng.integers(-8, 9, n + g).astype(np.float64)
    layout = pm.Layout(n, g)
    v = _vec(pm, layout, x)
    v.remove_mean()
    assert np.array_equal(v.data_copy(), x - x[:n].sum() / n)


def test_remove_mean_in_a_graph(pm):
    n = 1000
    x = np.random.default_rng(5).integers(-8, 9, n).astype(np.float64)
    layout = pm.Layout(n)
    v = _vec(pm, layout, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            v.remove_mean()
    torch.cuda.current_stream().wait_stream(side)
    v.data[:n].copy_(torch.from_numpy(x))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(v.data_copy(), x - x.sum() / n)


# ---- the singular operator ----------------------------------------------------------------------------------------


class Singular:
    """A matrix-free operator with an all-zero marker, the oracle's, and x_tight for one right-hand side."""

    def __init__(self, pm, P, n, wf, seed):
        from oracle import pmg_oracle as po

        self.pm, self.P = pm, P
        self.part = pm.BoxPartition(n, warp=MAPS[wf])
        self.lv = self.part.level(P)
        self.layout = pm.make_layout(self.lv)
        self.bc = np.zeros(self.lv.ndofs, dtype=np.int8)
        self.kappa = _kappa(P, self.part.ncells, 300 + seed)
        self.op = pm.MatFreeLaplacian(P, self.kappa, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap,
                                      self.lv.lcells, self.lv.bcells, self.bc, self.layout)
        self.op.compute_diag_inverse()
        self.A = po.Laplacian(P, self.kappa, self.lv.dofmap, self.part.xgeom, self.part.geom_dofmap, self.bc)
        self.dinv = self.A.diag_inverse()
        b = np.random.default_rng(seed).standard_normal(self.lv.ndofs)
        self.b = b - b.mean()
        nd = self.lv.ndofs
        assert nd <= DENSE_MAX
        M = np.empty((nd, nd))
        e = np.zeros(nd)
        for j in range(nd):
            e[j] = 1.0
            M[:, j] = self.A.apply(e)
            e[j] = 0.0
        self.x_tight = np.linalg.pinv(M, hermitian=True) @ self.b

    def jacobi(self, r):
        return self.dinv * r

    def solve(self, b, mode="constant", rtol=1e-10, max_iter=1000, operator=None, cg=None, x0=None):
        pm = self.pm
        cg = pm.CGSolver(self.layout) if cg is None else cg
        cg.set_max_iterations(max_iter)
        cg.set_tolerance(rtol)
        cg.set_nullspace(mode)
        x = _vec(pm, self.layout, np.zeros(self.lv.ndofs) if x0 is None else x0)
        its = cg.solve(self.op if operator is None else operator, x, _vec(pm, self.layout, b))
        return x.data_copy(), its


SHAPES = [(1, 6, None), (2, 3, "warp"), (4, 2, "twist")]
_singular = {}


def _case(pm, P, n, wf):
    key = (P, n, wf)
    if key not in _singular:
        _singular[key] = Singular(pm, P, n, wf, 10 * P + n)
    return _singular[key]


def _tolerance_rule(what, x_gpu, x_ref, x_tight):
    e_ref, e_gpu = _rel2(x_ref, x_tight), _rel2(x_gpu, x_tight)
    msg = f"{what}: e_ref = {e_ref:.3e}, device {e_gpu:.3e}, bound {10 * e_ref + 1e-12:.3e}"
    print(msg)
    assert e_gpu <= 10 * e_ref + 1e-12, msg
    return e_ref, e_gpu


# ---- 2. Jacobi CG -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("P,n,wf", SHAPES)
def test_jacobi_cg_on_the_singular_operator(pm, P, n, wf):
    c = _case(pm, P, n, wf)
    rtol = 1e-10
    x_ref, its_ref = ns.pcg_nullspace(c.A.apply, c.jacobi, c.b, np.zeros_like(c.b), rtol, 1000)
    x, its = c.solve(c.b, rtol=rtol)
    print(f"P = {P}, n = {n}: {its} iterations (restatement {its_ref})")
    assert abs(its - its_ref) <= 1
    assert _mean_is_zero(x)
    _tolerance_rule(f"P = {P} Jacobi", x, x_ref, c.x_tight)
    # an incompatible right-hand side is projected, not diverged on
    xs, its_s = c.solve(c.b + 0.7, rtol=rtol)
    assert abs(its_s - its_ref) <= 1 and _mean_is_zero(xs)
    _tolerance_rule(f"P = {P} Jacobi, b + 0.7", xs, x_ref, c.x_tight)
    # ... and a constant in the initial guess does not survive
    x0, its_0 = c.solve(c.b, rtol=rtol, x0=np.full(c.lv.ndofs, 2.5))
    assert abs(its_0 - its_ref) <= 1 and _mean_is_zero(x0)
    _tolerance_rule(f"P = {P} Jacobi, x0 = 2.5", x0, x_ref, c.x_tight)


def test_jacobi_cg_through_the_assembled_operator(pm):
    P, n, wf = SHAPES[1]
    c = _case(pm, P, n, wf)
    M = pm.MatrixOperator(c.op)
    x_ref, its_ref = ns.pcg_nullspace(c.A.apply, c.jacobi, c.b, np.zeros_like(c.b), 1e-10, 1000)
    x, its = c.solve(c.b + 0.7, operator=M)
    assert abs(its - its_ref) <= 1 and _mean_is_zero(x)
    _tolerance_rule("MatrixOperator Jacobi", x, x_ref, c.x_tight)


@pytest.mark.parametrize("P,n,wf", SHAPES)
def test_mode_set_and_unset_is_the_plain_solver(pm, P, n, wf):
    c = _case(pm, P, n, wf)
    never, its0 = c.solve(c.b, mode=None, rtol=0.0, max_iter=12)
    cg = pm.CGSolver(c.layout)
    cg.set_nullspace("constant")
    assert cg.nullspace() == "constant"
    toggled, its1 = c.solve(c.b, mode=None, rtol=0.0, max_iter=12, cg=cg)
    assert cg.nullspace() is None
    assert its0 == its1 == 12
    assert np.abs(toggled - never).max() <= NOISE * np.abs(never).max()


def test_lanczos_coefficients_are_those_of_the_projected_iteration(pm):
    """alpha_k and beta_k of the restatement: the Lanczos record follows the projected recurrences."""
    P, n, wf = SHAPES[0]
    c = _case(pm, P, n, wf)
    cg = pm.CGSolver(c.layout)
    cg.store_coefficients(True)
    c.solve(c.b + 0.7, rtol=0.0, max_iter=10, cg=cg)
    N = c.b.size
    r = ns.remove_mean(c.b + 0.7)
    z = c.jacobi(r)
    rz = ns.projected_rz(r @ z, r.sum(), z.sum(), N)
    p = z - z.sum() / N
    alphas, betas = [], []
    for _ in range(10):
        y = c.A.apply(p)
        alphas.append(rz / (p @ y))
        r = r - alphas[-1] * y
        z = c.jacobi(r)
        rz_new = ns.projected_rz(r @ z, r.sum(), z.sum(), N)
        betas.append(rz_new / rz)
        rz = rz_new
        p = betas[-1] * p + (z - z.sum() / N)
    assert np.abs(cg.alphas() / np.array(alphas) - 1).max() < 1e-9
    assert np.abs(cg.betas() / np.array(betas) - 1).max() < 1e-9


# ---- 3. PCG with the V-cycle --------------------------------------------------------------------------------------


class Hierarchy:
    """A p-multigrid hierarchy without a marked dof, the oracle's levels, and the tight solution of one system."""

    def __init__(self, pm, n, orders):
        from oracle import pmg_oracle as po

        self.pm, self.n, self.orders = pm, n, orders
        self.h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=bd.warp, dirichlet=_nowhere)
        h = self.h
        assert all(lv.bc_marker.sum() == 0 for lv in h.levels)
        part = h.part
        self.ops = [po.Laplacian(P, 0.05, lv.dofmap, part.xgeom, part.geom_dofmap, np.zeros(lv.ndofs, np.int8))
                    for P, lv in zip(orders, h.levels)]
        self.sm = [po.Chebyshev(e, 3) for e in h.eig_ranges]
        self.it = [po.Interpolator(orders[i], orders[i + 1], self.ops[i].dofmap, self.ops[i + 1].dofmap,
                                   self.ops[i].ndofs, self.ops[i + 1].ndofs) for i in range(len(orders) - 1)]
        self.b = h.rhs[-1].data_copy()
        self.amg_levels = None
        self.tight = {}

    def cycle(self, coarse=None):
        from oracle import pmg_oracle as po

        mg = po.MultigridPreconditioner(self.ops, self.sm, self.it, self.ops[0].bc, coarse_solver=coarse)
        return lambda r: mg.apply(r, np.zeros_like(r))

    def exported(self, amg):
        L = amg.num_levels()
        return ([amg.export(l, "A") for l in range(L)], [amg.export(l, "P") for l in range(L - 1)],
                [amg.level_info(l)["lambda_max"] for l in range(L)])

    def reference(self, variant, M, rtol, flexible):
        A = self.ops[-1]
        if variant not in self.tight:
            self.tight[variant] = ns.pcg_nullspace(A.apply, M, self.b, np.zeros_like(self.b), 1e-14, 200, flexible)[0]
        x_ref, its_ref = ns.pcg_nullspace(A.apply, M, self.b, np.zeros_like(self.b), rtol, 200, flexible)
        return x_ref, its_ref, self.tight[variant]

    def solve(self, rtol, flexible):
        pm, h = self.pm, self.h
        cg = pm.CGSolver(h.layouts[-1])
        cg.set_max_iterations(200)
        cg.set_tolerance(rtol)
        cg.set_flexible(flexible)
        cg.set_nullspace("constant")
        x = h.new_vector()
        x.set(0.0)
        its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
        return x.data_copy(), its


_hierarchies = {}


def _hier(pm, n, orders):
    if (n, orders) not in _hierarchies:
        _hierarchies[(n, orders)] = Hierarchy(pm, n, orders)
    return _hierarchies[(n, orders)]


VSHAPES = [(4, (1, 2, 4)), (12, (1, 2))]
RTOL_V = 1e-8


@pytest.mark.parametrize("variant", ["smoother", "flexible-cg", "amg-2-cycles", "amg-krylov"])
@pytest.mark.parametrize("n,orders", VSHAPES, ids=["4-2-1@4", "2-1@12"])
def test_pcg_with_the_vcycle(pm, n, orders, variant):
    H = _hier(pm, n, orders)
    h, A0 = H.h, H.ops[0]
    flexible = variant in ("flexible-cg", "amg-krylov")
    h.mg.set_precision("fp64")
    h.mg.set_graph(False)
    keep = None
    if variant == "smoother":
        h.mg.set_coarse_solver(None)
        M = H.cycle()
    elif variant == "flexible-cg":
        keep = pm.CGSolver(h.layouts[0])
        keep.set_max_iterations(40)
        keep.set_tolerance(1e-4)
        keep.set_nullspace("constant")
        h.mg.set_coarse_solver(keep)
        dinv0 = A0.diag_inverse()

        def coarse(u0, b0):
            u0[:] = ns.pcg_nullspace(A0.apply, lambda r: dinv0 * r, b0, np.zeros_like(b0), 1e-4, 40)[0]

        M = H.cycle(coarse)
    else:
        keep = pm.AmgSolver(h.operators[0], cycles=2) if variant == "amg-2-cycles" else pm.AmgSolver(h.operators[0])
        keep.set_nullspace("constant")
        assert keep.num_levels() == (1 if n == 4 else 2)
        h.mg.set_coarse_solver(keep)
        As, Ps, rhos = H.exported(keep)
        cyc = ns.NullspaceAmgCycle(As, Ps, rhos)
        if variant == "amg-2-cycles":
            def coarse(u0, b0):
                u0[:] = cyc.stationary(b0, 2)
        else:
            def coarse(u0, b0):
                u0[:] = cyc.pcg(A0.apply, b0, 1e-5, 60)[0]
        M = H.cycle(coarse)
    try:
        x_ref, its_ref, x_tight = H.reference(variant, M, RTOL_V, flexible)
        x, its = H.solve(RTOL_V, flexible)
        print(f"n = {n}, orders {orders}, {variant}: {its} iterations (restatement {its_ref})")
        assert abs(its - its_ref) <= 1
        assert _mean_is_zero(x)
        _tolerance_rule(f"{orders}@{n} {variant}", x, x_ref, x_tight)
        if variant in ("smoother", "amg-2-cycles"):  # capturable: replay against eager
            h.mg.set_graph(True)
            n0 = h.mg.graph_replays()
            xg, its_g = H.solve(RTOL_V, flexible)
            assert h.mg.graph_replays() > n0
            g = np.abs(xg - x).max() / np.abs(x).max()
            print(f"    graph replay against eager {g:.3e}")
            assert its_g == its and g <= 1e-12
    finally:
        h.mg.set_graph(False)
        h.mg.set_coarse_solver(None)


def test_pcg_with_the_fp32_cycle(pm):
    n, orders = VSHAPES[0]
    H = _hier(pm, n, orders)
    h = H.h
    h.mg.set_coarse_solver(None)
    try:
        x_ref, its_ref, x_tight = H.reference("smoother", H.cycle(), RTOL_V, False)
        h.mg.set_precision("fp32")
        h.mg.set_graph(False)
        x, its = H.solve(RTOL_V, False)
        print(f"FP32 cycle: {its} iterations (FP64 restatement {its_ref})")
        assert abs(its - its_ref) <= 1
        assert _mean_is_zero(x)
        _tolerance_rule("FP32 cycle", x, x_ref, x_tight)
        h.mg.set_graph(True)
        xg, its_g = H.solve(RTOL_V, False)
        g = np.abs(xg - x).max() / np.abs(x).max()
        print(f"    graph replay against eager {g:.3e}")
        assert g <= 1e-6
    finally:
        h.mg.set_graph(False)
        h.mg.set_precision("fp64")


# ---- 4. the AMG alone ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,levels", [(6, 1), (10, 2), (32, 3)])
def test_amg_alone(pm, n, levels):
    from oracle import pmg_oracle as po

    part = pm.BoxPartition(n, warp=bd.warp)
    lv = part.level(1)
    layout = pm.make_layout(lv)
    bc = np.zeros(lv.ndofs, dtype=np.int8)
    op = pm.MatFreeLaplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bc, layout)
    op.compute_diag_inverse()
    amg = pm.AmgSolver(op, max_iter=60, rtol=1e-8)
    assert amg.num_levels() == levels

    def exported():
        out = []
        for l in range(levels):
            for which in ("A", "P")[: 2 if l + 1 < levels else 1]:
                m = amg.export(l, which)
                out += [m.indptr.tobytes(), m.indices.tobytes(), m.data.tobytes()]
        return out

    before = exported()
    As = [amg.export(l, "A") for l in range(levels)]
    Ps = [amg.export(l, "P") for l in range(levels - 1)]
    rhos = [amg.level_info(l)["lambda_max"] for l in range(levels)]
    cyc = ns.NullspaceAmgCycle(As, Ps, rhos)
    b = np.random.default_rng(n).standard_normal(lv.ndofs)
    b -= b.mean()
    want = cyc.cycle_projected(b)
    x, bv = pm.Vector(layout), _vec(pm, layout, b)
    if n == 10:  # without the mode the hierarchy does not reproduce the restated cycle: its last level is singular
        amg.cycle(x, bv)
        plain = x.data_copy()
        away = np.abs(plain - want).max() / np.abs(want).max()
        print(f"n = {n}: the cycle without the mode is {away:.3e} away from the restated one")
        assert not away <= 1e-8
    amg.set_nullspace("constant")
    assert amg.nullspace() == "constant"
    assert exported() == before
    amg.cycle(x, bv)
    got = x.data_copy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"n = {n}, {levels} level(s), coarsest {As[-1].shape[0]} rows: cycle against numpy {err:.3e}")
    assert err <= 1e-11
    assert _mean_is_zero(got)
    # Krylov mode
    A = po.Laplacian(1, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, bc)
    x_ref, its_ref = cyc.pcg(A.apply, b, 1e-8, 60)
    its = amg.solve(x, bv)
    print(f"    Krylov mode: {its} iterations (restatement {its_ref})")
    assert abs(its - its_ref) <= 1 and _mean_is_zero(x.data_copy())
    x_tight = ns.pcg_nullspace(A.apply, cyc.cycle, b, np.zeros_like(b), 1e-14, 200)[0]
    _tolerance_rule(f"AMG Krylov n = {n}", x.data_copy(), x_ref, x_tight)
    # stationary mode: the solve ends with the mean removed too
    st = pm.AmgSolver(op, cycles=2)
    st.set_nullspace("constant")
    st.solve(x, bv)
    want2 = cyc.stationary(b, 2)
    assert np.abs(x.data_copy() - want2).max() <= 1e-11 * np.abs(want2).max() and _mean_is_zero(x.data_copy())
    # back to NONE: the plain inverse again
    if n == 10:
        amg.set_nullspace(None)
        amg.cycle(x, bv)
        assert np.abs(x.data_copy() - plain).max() <= NOISE * np.abs(plain).max() or not np.isfinite(plain).all()


# ---- 5. refusals --------------------------------------------------------------------------------------------------


def test_refusals_and_the_solve_after_them(pm):
    from pmg_dolfinx_amd._lib import PmgError

    P, n, wf = SHAPES[1]
    c = _case(pm, P, n, wf)
    part, lv, layout = c.part, c.lv, c.layout
    cg = pm.CGSolver(layout)
    cg.set_max_iterations(1000)
    cg.set_tolerance(1e-10)
    with pytest.raises(PmgError, match="unknown mode 5"):
        cg.set_nullspace(5)
    assert cg.nullspace() is None
    cg.set_nullspace("constant")
    x, b = pm.Vector(layout), _vec(pm, layout, c.b)
    # a marked row
    marked = pm.MatFreeLaplacian(P, c.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells,
                                 lv.bc_marker, layout)
    marked.compute_diag_inverse()
    with pytest.raises(PmgError, match=r"pmg_cg_solve: .*marked \(Dirichlet\) rows"):
        cg.solve(marked, x, b)
    with pytest.raises(PmgError, match=r"pmg_cg_solve_matrix: .*marked \(Dirichlet\) rows"):
        cg.solve(pm.MatrixOperator(marked), x, b)
    # a reaction term, a Robin term
    other = pm.MatFreeLaplacian(P, c.kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, c.bc, layout)
    other.set_reaction(np.full(part.ncells, 0.5))
    other.compute_diag_inverse()
    with pytest.raises(PmgError, match="reaction term"):
        cg.solve(other, x, b)
    other.set_reaction(None)
    cells, facets = part.exterior_facets()
    other.set_robin(cells, facets, np.full((cells.size, (P + 1) ** 2), 0.25))
    with pytest.raises(PmgError, match="Robin term"):
        cg.solve(other, x, b)
    # the AMG: a marked operator, an unknown mode, a reaction term, a Robin term, the replicated and the distributed form
    p1 = part.level(1)
    l1 = pm.make_layout(p1)
    op1m = pm.MatFreeLaplacian(1, 2.0, p1.dofmap, part.xgeom, part.geom_dofmap, p1.lcells, p1.bcells, p1.bc_marker, l1)
    op1m.compute_diag_inverse()
    amg = pm.AmgSolver(op1m)
    with pytest.raises(PmgError, match=r"pmg_amg_set_nullspace: .*marked"):
        amg.set_nullspace("constant")
    assert amg.nullspace() is None
    with pytest.raises(PmgError, match="unknown mode -3"):
        amg.set_nullspace(-3)
    op1 = pm.MatFreeLaplacian(1, 2.0, p1.dofmap, part.xgeom, part.geom_dofmap, p1.lcells, p1.bcells,
                              np.zeros(p1.ndofs, np.int8), l1)
    op1.compute_diag_inverse()
    op1.set_reaction(np.full(part.ncells, 0.5))
    with pytest.raises(PmgError, match=r"pmg_amg_set_nullspace: .*reaction term"):
        pm.AmgSolver(op1).set_nullspace("constant")
    op1.set_reaction(None)
    op1.set_robin(cells, facets, np.full((cells.size, 4), 0.25))
    with pytest.raises(PmgError, match=r"pmg_amg_set_nullspace: .*Robin term"):
        pm.AmgSolver(op1).set_nullspace("constant")
    op1.set_robin(cells, facets, None)
    assert not op1.has_robin() and not op1.has_reaction()
    gi = np.arange(p1.ndofs, dtype=np.int64)
    for setup in ("gathered", "distributed"):  # pmg_amg_create_replicated, pmg_amg_create_distributed
        form = pm.AmgSolver(op1, global_index=gi, n_global=p1.ndofs, setup=setup)
        with pytest.raises(PmgError, match="replicated and distributed"):
            form.set_nullspace("constant")
        assert form.nullspace() is None
    # a term attached AFTER the mode was set is refused where the AMG solves, not projected; removing it restores
    x1, b1 = pm.Vector(l1), pm.Vector(l1)
    g1 = np.random.default_rng(8).standard_normal(p1.ndofs)
    b1.data.copy_(torch.from_numpy(g1 - g1.mean()))
    good = pm.AmgSolver(op1)
    good.set_nullspace("constant")
    good.cycle(x1, b1)
    before = x1.data_copy()
    op1.set_reaction(np.full(part.ncells, 0.5))
    with pytest.raises(PmgError, match=r"pmg_amg_cycle: .*reaction term"):
        good.cycle(x1, b1)
    with pytest.raises(PmgError, match=r"pmg_amg_solve: .*reaction term"):
        good.solve(x1, b1)
    op1.set_reaction(None)
    good.cycle(x1, b1)
    assert np.abs(x1.data_copy() - before).max() <= NOISE * np.abs(before).max()
    # the valid solve after all of it
    x_ref, its_ref = ns.pcg_nullspace(c.A.apply, c.jacobi, c.b, np.zeros_like(c.b), 1e-10, 1000)
    x.set(0.0)
    its = cg.solve(c.op, x, b)
    assert abs(its - its_ref) <= 1
    _tolerance_rule("after the refusals", x.data_copy(), x_ref, c.x_tight)


def test_coarse_cg_inside_a_multigrid_honours_its_own_refusals(pm):
    """A pmg_cg installed with pmg_multigrid_set_coarse_solver goes through pmg_cg_solve: with its mode on, a level-0
    operator with a marked row, a reaction term or a Robin term is refused from inside the cycle, with the message of
    pmg_cg_solve -- and the solves before and after the refusals agree."""
    from pmg_dolfinx_amd._lib import PmgError

    n, orders = 4, (1, 2)

    def coarse_cg(h, mode):
        cg = pm.CGSolver(h.layouts[0])
        cg.set_max_iterations(30)
        cg.set_tolerance(1e-4)
        cg.set_nullspace(mode)
        h.mg.set_coarse_solver(cg)
        return cg

    def cycle(h):
        v = h.new_vector()
        v.set(0.0)
        h.mg.apply(h.rhs[-1], v)
        return v.data_copy()

    # a marked level-0 operator (the whole boundary is Dirichlet)
    hm = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=bd.warp)
    assert hm.levels[0].bc_marker.sum() > 0
    hm.mg.set_graph(False)
    cg = coarse_cg(hm, None)
    before = cycle(hm)
    cg.set_nullspace("constant")
    with pytest.raises(PmgError, match=r"pmg_cg_solve: .*marked \(Dirichlet\) rows"):
        cycle(hm)
    cg.set_nullspace(None)
    after = cycle(hm)
    assert np.abs(after - before).max() <= NOISE * np.abs(before).max()
    hm.mg.set_coarse_solver(None)

    # an unmarked hierarchy: valid with the mode on; a reaction or Robin term on level 0 is refused
    h = pm.PoissonHierarchy(n, orders, kappa=0.05, cheb_its=3, warp=bd.warp, dirichlet=_nowhere)
    h.mg.set_graph(False)
    cg = coarse_cg(h, "constant")
    outer = pm.CGSolver(h.layouts[-1])
    outer.set_max_iterations(100)
    outer.set_tolerance(1e-8)
    outer.set_flexible(True)
    outer.set_nullspace("constant")

    def solve():
        x = h.new_vector()
        x.set(0.0)
        its = outer.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
        return x.data_copy(), its

    x_before, its_before = solve()
    assert 0 < its_before < 100 and _mean_is_zero(x_before)
    op0, part = h.operators[0], h.part
    cells, facets = part.exterior_facets()
    op0.set_reaction(np.full(part.ncells, 0.5))
    with pytest.raises(PmgError, match=r"pmg_cg_solve: .*reaction term"):
        solve()
    op0.set_reaction(None)
    op0.set_robin(cells, facets, np.full((cells.size, 4), 0.25))
    with pytest.raises(PmgError, match=r"pmg_cg_solve: .*Robin term"):
        solve()
    op0.set_robin(cells, facets, None)
    x_after, its_after = solve()
    assert its_after == its_before
    assert np.abs(x_after - x_before).max() <= NOISE * np.abs(x_before).max()
    h.mg.set_coarse_solver(None)


def test_remove_mean_refuses_weights_of_another_size(pm):
    x, w = pm.Vector(pm.Layout(100)), pm.Vector(pm.Layout(60))
    with pytest.raises(RuntimeError, match="Incompatible vector sizes"):
        x.remove_mean(w)


# ---- 6. two ranks sharing the one GPU -----------------------------------------------------------------------------


def _rank_body(rank, world, port, n, dims, P):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm

        torch.cuda.set_device(0)
        H = pm.PoissonHierarchy(n, (P,), kappa=0.05, cheb_its=3, proc_dims=dims, rank=rank, size=world, warp=bd.warp,
                                dirichlet=_nowhere)
        lv, layout, op = H.levels[-1], H.layouts[-1], H.operators[-1]
        l2g = lv.local_to_global
        nglob = H.part.global_ndofs(P)
        g = np.random.default_rng(21).standard_normal(nglob)
        v = pm.Vector(layout)
        v.data.copy_(torch.from_numpy(g[l2g]))
        v.remove_mean()
        out = {"l2g": l2g[: lv.size_local], "removed": v.data_copy(), "all": l2g}
        b = g - g.mean()
        cg = pm.CGSolver(layout)
        cg.set_max_iterations(1000)
        cg.set_tolerance(1e-10)
        cg.set_nullspace("constant")
        x, bv = pm.Vector(layout), pm.Vector(layout)
        x.set(0.0)
        bv.data.copy_(torch.from_numpy((b + 0.7)[l2g]))
        out["its"] = cg.solve(op, x, bv)
        out["x"] = x.data_copy()[: lv.size_local]
        return out
    finally:
        dist.destroy_process_group()


def _rank_worker(rank, world, port, *args):
    from test_gpu_distributed import _reporting

    _reporting(_rank_body)(rank, world, port, *args)


def test_two_ranks(built):
    from oracle import pmg_oracle as po

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_distributed import _run_ranks

    n, dims, P = 4, (2, 1, 1), 2
    res = _run_ranks(_rank_worker, 2, (n, dims, P), timeout=120)
    mesh = po.BoxMesh(n, warp=bd.warp)
    A = po.Laplacian(P, 0.05, mesh.dofmap(P), mesh.xgeom, mesh.geom_dofmap, np.zeros(mesh.ndofs(P), np.int8))
    nd = A.ndofs
    g = np.random.default_rng(21).standard_normal(nd)
    want = ns.remove_mean(g)
    for r in res:  # owned and ghost entries alike
        assert np.abs(r["removed"] - want[r["all"]]).max() <= nd * EPS * np.abs(g).max()
    b = g - g.mean()
    dinv = A.diag_inverse()
    x_ref, its_ref = ns.pcg_nullspace(A.apply, lambda r: dinv * r, b, np.zeros(nd), 1e-10, 1000)
    M = np.empty((nd, nd))
    e = np.zeros(nd)
    for j in range(nd):
        e[j] = 1.0
        M[:, j] = A.apply(e)
        e[j] = 0.0
    x_tight = np.linalg.pinv(M, hermitian=True) @ b
    x = np.empty(nd)
    for r in res:
        x[r["l2g"]] = r["x"]
        assert abs(r["its"] - its_ref) <= 1
    assert res[0]["its"] == res[1]["its"]
    _tolerance_rule("two ranks, Jacobi", x, x_ref, x_tight)
