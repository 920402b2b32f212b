"""The AMG set-up of csrc/amg.hip pinned to its independent restatement (oracle/amg_oracle.py: ``aggregate``,
``smoothed_prolongator``, ``power_bound``, ``build``), level by level, on meshes chosen to reach each branch: one, two
and three levels, several host row blocks, rows left out of the coarse space, short rows -- and every lane width of
the CSR product.  On the same exported hierarchies the device cycle and the stationary solve are compared with the
numpy cycle.  Then the replicated form under a permuted global numbering, and the hierarchy's independence of the
number of host threads.

Measured on the MI355X (rho_l / lambda_max(D^-1 A_l) per level, rho_l = 1.05 x 20 power steps; below 1 means the
smoother's bound sits under the true largest eigenvalue):
  case         level sizes        lane widths A / P / R            rho_l / lambda_max per level
  one-level    729                4 / - / -                        1.0073
  two-levels   2197, 183          8, 32 / 4 / 32                   1.0005, 1.0169
  flat         3375, 845, 247     8, 32, 32 / 4, 16 / 16, 32       1.0328, 1.0297, 1.0133
  row-blocks   9261, 849, 103     8, 32, 32 / 4, 8 / 32, 32        (9261 rows: not computed), 0.9886, 1.0492
  kappa-jump   3375, 302          8, 32 / 4 / 32                   1.0102, 0.9967
  unwarped     2197, 183          8, 16 / 2 / 16                   1.0010, 1.0171
  two-layers   1156, 86           4, 16 / 2 / 16                   1.0148, 1.0128
  slab         867, 43            2, 8 / 2 / 8                     1.0273, 1.0360
Pass 3 of the aggregation made no aggregate in any case (see tests/test_amg_oracle.py for why it cannot, with a
symmetric strength graph); the kappa-jump case leaves 5 interior rows out of the coarse space, row-blocks 3 rows of
level 1.  The device cycle and the stationary solve differ from numpy by at most 2e-15 max|want|, three levels included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_BLOCK = 4096  # rows per block of the host set-up's threaded loops


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


def flat_twist(x):
    return twist(x) * np.array([1.0, 1.0, 0.04])


def _jump(ncells):
    return np.where(np.random.default_rng(7).random(ncells) < 0.5, 1.0, 1e4)


# name: (cells, warp, kappa (a number, or a function of the number of cells), levels it must reach)
CASES = {
    "one-level": (8, twist, 2.0, 1),            # 729 rows: the dense inverse alone
    "two-levels": (12, twist, 2.0, 2),          # 2197 rows
    "flat": (14, flat_twist, 2.0, 3),           # 3375 rows, cells 25 times wider than high: line aggregates, dense P_1
    "row-blocks": (20, twist, 2.0, 3),          # 9261 rows = three row blocks of the host loops
    "kappa-jump": (14, twist, _jump, 2),        # interior rows with no strong coupling stay out of the coarse space
    "unwarped": (12, None, 2.0, 2),             # axis-parallel cells: the off-axis couplings are explicit zeros
    "two-layers": ((16, 16, 3), twist, 2.0, 2),  # 1156 rows, two interior layers, 7.0 entries per row of A_0: width 4
    "slab": ((16, 16, 2), twist, 2.0, 2),       # 867 rows, one interior layer, 2.9 entries per row: lane width 2
}

_products_run = set()  # (lane width, mode) of every CSR product the device work of the cases below has launched
_cache = {}


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _p1(pm, n, warp=twist, kappa=2.0):
    part = pm.BoxPartition(n, warp=warp)
    lv = part.level(1)
    layout = pm.make_layout(lv)
    if callable(kappa):
        kappa = kappa(lv.dofmap.shape[0])
    op = pm.MatFreeLaplacian(1, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    op.compute_diag_inverse()
    return part, lv, layout, op, kappa


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


def lane_width(nnz, rows):
    """The rule of upload_csr: lanes per row from the average row length."""
    avg = nnz / rows if rows else 1.0
    return 32 if avg > 48 else 16 if avg > 24 else 8 if avg > 10 else 4 if avg > 4 else 2


class _Hierarchy:
    """One case: the operator, the library's exported hierarchy (shared by the tests, never modified)."""

    def __init__(self, pm, name):
        n, warp, kappa, self.want_levels = CASES[name]
        self.part, self.lv, self.layout, self.op, self.kappa = _p1(pm, n, warp, kappa)
        self.amg = pm.AmgSolver(self.op)
        self.L = self.amg.num_levels()
        self.As = [self.amg.export(l, "A") for l in range(self.L)]  # explicit zeros kept
        self.Ps = [self.amg.export(l, "P") for l in range(self.L - 1)]
        self.rhos = [self.amg.level_info(l)["lambda_max"] for l in range(self.L)]
        self.bc = self.lv.bc_marker.astype(bool)


def _hier(pm, name):
    if name not in _cache:
        _cache[name] = _Hierarchy(pm, name)
    return _cache[name]


def _lambda_true(A):
    d = A.diagonal()
    return float(np.linalg.eigvalsh(A.toarray() / np.sqrt(np.outer(d, d)))[-1])  # D^-1 A ~ D^-1/2 A D^-1/2


@pytest.mark.parametrize("name", list(CASES))
def test_level_zero_and_what_the_case_reaches(pm, name):
    from oracle import pmg_oracle as po

    h = _hier(pm, name)
    ref = po.Laplacian(1, h.kappa, h.lv.dofmap, h.part.xgeom, h.part.geom_dofmap, h.lv.bc_marker).assemble_csr()
    assert abs(h.As[0] - ref).max() < 1e-12 * abs(ref).max()
    sizes = [A.shape[0] for A in h.As]
    assert sizes == [h.amg.level_info(l)["rows"] for l in range(h.L)]
    print(f"{name}: level sizes {sizes}")
    assert h.L == h.want_levels and sizes[-1] <= 800
    if name == "row-blocks":
        assert sizes[0] > 2 * ROW_BLOCK  # three row blocks: the threaded loops of the set-up
    if name == "unwarped":
        assert (h.As[0].data == 0.0).sum() > h.As[0].shape[0]  # explicit zeros in A_0


@pytest.mark.parametrize("name", list(CASES))
def test_prolongators_equal_the_restatement(pm, name):
    from oracle import amg_oracle as ao

    h = _hier(pm, name)
    for l in range(h.L - 1):
        A, P = h.As[l], h.Ps[l]
        st = {}
        agg, na = ao.aggregate(A, 0.08 / 2 ** l, st)
        sizes = np.bincount(agg[agg >= 0], minlength=na)
        interior_outside = int((agg < 0).sum() - (h.bc.sum() if l == 0 else 0))
        print(f"{name} level {l}: {na} aggregates of {sizes.min()}..{sizes.max()} rows (median {np.median(sizes):.0f}), "
              f"pass-3 roots {st['pass3_roots']}, rows outside the coarse space {st['outside']} "
              f"({interior_outside} of them no Dirichlet rows), P: {P.nnz / P.shape[0]:.1f} entries per row")
        assert P.shape == (A.shape[0], na)
        want = ao.smoothed_prolongator(A, agg, na, h.rhos[l])
        assert abs(P - want).max() <= 1e-13 * abs(want).max()
        # the library stores no zero of P, and no row outside the coarse space has an entry
        assert (P.data != 0.0).all() and np.diff(P.indptr)[agg < 0].sum() == 0
        assert np.array_equal(np.unique(P.indices), np.arange(na))
        if l == 0:
            assert (agg[h.bc] == -1).all()
            if name == "kappa-jump":
                assert interior_outside > 0
            else:
                assert interior_outside == 0
        if name == "flat" and l == 0:
            assert np.median(sizes) <= 3  # line aggregates along the short direction


@pytest.mark.parametrize("name", list(CASES))
def test_smoothing_bounds_equal_the_restated_power_method(pm, name):
    from oracle import amg_oracle as ao

    h = _hier(pm, name)
    for l, (A, rho) in enumerate(zip(h.As, h.rhos)):
        want = 1.05 * ao.power_bound(A)
        assert abs(rho - want) <= 1e-11 * want, (l, rho, want)
        if A.shape[0] <= 6000:
            lam = _lambda_true(A)
            print(f"{name} level {l}: rho / lambda_max(D^-1 A) = {rho / lam:.4f}")
            assert rho <= 1.05 * lam * (1 + 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_levels_equal_the_restated_build(pm, name):
    from oracle import amg_oracle as ao

    h = _hier(pm, name)
    As, Ps, rhos, stats = ao.build(h.As[0])
    assert len(As) == h.L
    assert [A.shape[0] for A in As] == [A.shape[0] for A in h.As]
    for l in range(h.L):  # the restated hierarchy itself: Galerkin operators and bounds agree to rounding
        assert abs(As[l] - h.As[l]).max() < 1e-12 * abs(h.As[l]).max()
        assert abs(rhos[l] - h.rhos[l]) < 1e-10 * h.rhos[l]
    print(f"{name}: pass-3 roots per coarsening {[s['pass3_roots'] for s in stats]}")


def _record(h, stationary):
    """(lane width, mode) of the products one cycle (and the residual of a stationary solve) launches."""
    for l in range(h.L - 1):
        A, P = h.As[l], h.Ps[l]
        _products_run.add((lane_width(A.nnz, A.shape[0]), 0))  # the smoother's A x
        _products_run.add((lane_width(P.nnz, P.shape[1]), 0))  # R r, R = P^T
        _products_run.add((lane_width(P.nnz, P.shape[0]), 2))  # x += P x_c
    if stationary:
        _products_run.add((lane_width(h.As[0].nnz, h.As[0].shape[0]), 1))  # b - A x


def _device_work(pm, name):
    """Cycles with 1 and 3 smoother steps and three stationary cycles on the device against numpy on the exported
    hierarchy; the tolerance is the one of tests/test_gpu_amg.py, 1e-11 max|want|, at every depth.  Once per case."""
    from oracle.amg_oracle import AmgCycle

    h = _hier(pm, name)
    if getattr(h, "device_work_done", False):
        return
    rng = np.random.default_rng(1)
    b = rng.standard_normal(h.lv.ndofs)
    b[h.bc] = 0.0
    bv = _vec(pm, h.layout, b)
    widths = {"A": [lane_width(A.nnz, A.shape[0]) for A in h.As], "P": [lane_width(P.nnz, P.shape[0]) for P in h.Ps],
              "R": [lane_width(P.nnz, P.shape[1]) for P in h.Ps]}
    print(f"{name}: lane widths {widths}")
    for k in (1, 3):
        amg = pm.AmgSolver(h.op, smoother_iterations=k)
        assert amg.info() == h.amg.info()  # the same hierarchy every time it is built
        ref = AmgCycle(h.As, h.Ps, h.rhos, k)
        x = pm.Vector(h.layout)
        x.set(7.0)  # the cycle starts from zero whatever x holds
        amg.cycle(x, bv)
        want = ref.cycle(b)
        err = np.abs(x.data_copy() - want).max() / np.abs(want).max()
        print(f"{name}: cycle k = {k}: rel. difference {err:.2e}")
        assert err < 1e-11
        if h.L == 1:
            direct = np.linalg.solve(h.As[0].toarray(), b)
            assert np.abs(x.data_copy() - direct).max() < 1e-11 * np.abs(direct).max()
    _record(h, False)
    amg = pm.AmgSolver(h.op, cycles=3)
    ref = AmgCycle(h.As, h.Ps, h.rhos, 2)
    x = pm.Vector(h.layout)
    x.set(7.0)
    assert amg.solve(x, bv) == 3
    want = ref.stationary(b, 3)
    err = np.abs(x.data_copy() - want).max() / np.abs(want).max()
    print(f"{name}: three stationary cycles: rel. difference {err:.2e}")
    assert err < 1e-11
    _record(h, True)
    h.device_work_done = True


@pytest.mark.parametrize("name", list(CASES))
def test_device_cycle_and_stationary_solve_equal_numpy(pm, name):
    _device_work(pm, name)


def test_every_lane_width_of_the_csr_product_has_run(pm):
    """The widths are derived by upload_csr's rule from the exported matrices of the cases whose device work has
    been compared with numpy (done here for any case the tests above have not run)."""
    for name in CASES:
        _device_work(pm, name)
    print("products run (lane width, mode):", sorted(_products_run))
    assert {w for w, m in _products_run if m == 0} == {2, 4, 8, 16, 32}
    p_widths = {lane_width(P.nnz, P.shape[0]) for h in _cache.values() for P in h.Ps}
    assert p_widths and p_widths <= {w for w, m in _products_run if m == 2}
    assert {w for w, m in _products_run if m == 1} >= {2, 4, 8}  # b - A_0 x: A_0 of "slab", of "one-level" and "two-layers", of the others


# ---- the replicated form on one rank under a permuted global numbering -------------------------------------------
@pytest.mark.parametrize("fine_level", [False, True], ids=["replicated-solve", "distributed-fine-level"])
def test_replicated_form_with_a_permuted_global_numbering(pm, fine_level):
    """One rank whose global numbers are a random permutation of its local ones: a wrong index in the scatter to the
    global vector, in the read-back or in the gather of the rows cannot hide as it does behind the identity map.

    The gathered level-0 matrix is the oracle's, permuted.  Aggregation follows the row order, so the permuted
    hierarchy is another hierarchy than the unpermuted one (the restated set-up: 133 aggregates instead of 183, 8 CG
    iterations to 1e-8 instead of 7); what is the same is the solution, and the iteration count is the count of the
    same CG in numpy on the exported (permuted) hierarchy."""
    from oracle.amg_oracle import AmgCycle

    h = _hier(pm, "two-levels")
    N = h.lv.ndofs
    perm = np.random.default_rng(2024).permutation(N)  # local -> global
    assert (perm != np.arange(N)).sum() > 0.99 * N
    inv = np.argsort(perm)
    b = np.random.default_rng(11).standard_normal(N)
    b[h.bc] = 0.0
    bv = _vec(pm, h.layout, b)

    def solver(rtol):
        return pm.AmgSolver(h.op, max_iter=60, rtol=rtol, global_index=perm, n_global=N,
                            distributed_fine_level=fine_level)

    amg = solver(1e-8)
    Ag = amg.export(0, "A")
    want = h.As[0][inv][:, inv]  # Ag[perm[i], perm[j]] = A[i, j]
    assert abs(Ag - want).max() < 1e-12 * abs(want).max()
    L = amg.num_levels()
    assert L == 2
    As = [Ag] + [amg.export(l, "A") for l in range(1, L)]
    Ps = [amg.export(l, "P") for l in range(L - 1)]
    ref = AmgCycle(As, Ps, [amg.level_info(l)["lambda_max"] for l in range(L)], 2)
    xr, its_ref = ref.pcg(lambda v: Ag @ v, b[inv], 1e-8, 60)
    x = pm.Vector(h.layout)
    its = amg.solve(x, bv)
    plain = pm.AmgSolver(h.op, max_iter=60, rtol=1e-8)
    x0 = pm.Vector(h.layout)
    its_plain = plain.solve(x0, bv)
    print(f"iterations to 1e-8: permuted replicated {its}, numpy on its hierarchy {its_ref}, unpermuted {its_plain}")
    assert its == its_ref and its <= 14
    assert np.abs(x.data_copy() - xr[perm]).max() < 1e-8 * np.abs(xr).max()  # read back in local order
    # against the unpermuted, non-replicated solver: two hierarchies, one solution -- both solved to 1e-12, so that
    # what the two preconditioners leave differs by less than the 1e-9 asked
    amg, plain = solver(1e-12), pm.AmgSolver(h.op, max_iter=60, rtol=1e-12)
    amg.solve(x, bv)
    plain.solve(x0, bv)
    assert np.abs(x.data_copy() - x0.data_copy()).max() < 1e-9 * np.abs(x0.data_copy()).max()


# ---- the hierarchy does not depend on the number of host threads --------------------------------------------------
def test_hierarchy_is_byte_identical_for_any_number_of_host_threads(pm, tmp_path):
    """PMG_HOST_THREADS is read once per process: one fresh child per value, one after the other, each writing every
    exported array and every bound of the n = 20 hierarchy (three row blocks) as bytes."""
    script = os.path.join(HERE, "amg_hierarchy_dump.py")
    blobs = []
    for threads in (1, 3, 16):
        out = tmp_path / f"hierarchy_{threads}.bin"
        env = dict(os.environ, PMG_HOST_THREADS=str(threads))
        r = subprocess.run([sys.executable, script, "20", str(out)], env=env, capture_output=True, text=True,
                           timeout=180)
        assert r.returncode == 0, f"PMG_HOST_THREADS={threads}:\n{r.stdout}\n{r.stderr}"
        blobs.append(out.read_bytes())
        print(f"PMG_HOST_THREADS={threads}: {r.stdout.strip()}, {len(blobs[-1])} bytes")
    assert len(blobs[0]) > 8 * 9261 * 10
    assert blobs[1] == blobs[0] and blobs[2] == blobs[0]
    # ... and it is the hierarchy of this process (whatever its number of threads)
    from amg_hierarchy_dump import hierarchy_bytes

    assert hierarchy_bytes(_hier(pm, "row-blocks").amg) == blobs[0]
