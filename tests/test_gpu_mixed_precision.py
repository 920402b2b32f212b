"""Mixed precision: the FP32 V-cycle inside FP64 CG (pmg_multigrid_set_precision, pmg_laplacian_apply_f32).

The FP32 operator against the FP64 oracle at every degree (1e-5 relative, max norm), the FP32 cycle against the
oracle's FP64 cycle (1e-4), PCG and stationary cycles with the FP32 cycle reaching FP64 accuracy (no float floor),
graph replay, switching back and forth, a replaced diagonal, the refusals, and the driver's --fp32-cycle."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pmg-dolfinx_amd", "bin")


def warp(x):
    return x + 0.03 * np.sin(3.0 * x[:, [1, 2, 0]])


def twist(x):
    y = x.copy()
    y[:, 0] += 0.12 * x[:, 1] * x[:, 2]
    y[:, 1] += 0.10 * x[:, 0] * x[:, 2] + 0.05 * x[:, 0] * x[:, 1] * x[:, 2]
    y[:, 2] += 0.08 * x[:, 0] * x[:, 1]
    return y


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _fp32_apply(op, u):
    x = torch.from_numpy(u.astype(np.float32)).cuda()
    y = torch.full_like(x, 7.0)  # the apply overwrites its output
    op.apply_fp32(x, y)
    torch.cuda.synchronize()
    return y.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("merge", [None, 0, 1 << 40])
@pytest.mark.parametrize("bc", [True, False])
@pytest.mark.parametrize("mesh", [True, "twist"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_apply_parity_all_degrees(pm, P, mesh, bc, merge):
    from oracle import pmg_oracle as po

    n = (3, 2, 4) if P > 4 else (5, 4, 3)
    wf = {True: warp, "twist": twist}[mesh]
    if merge is not None:
        pm.set_merge_threshold(merge)
    try:
        part = pm.BoxPartition(n, warp=wf)
        lv = part.level(P)
        bcm = lv.bc_marker if bc else np.zeros_like(lv.bc_marker)
        layout = pm.make_layout(lv)
        op = pm.MatFreeLaplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, bcm, layout)
    finally:
        pm.set_merge_threshold(-1)
    A = po.Laplacian(P, 2.0, lv.dofmap, part.xgeom, part.geom_dofmap, bcm)
    u = np.random.default_rng(P).standard_normal(lv.ndofs)
    got = _fp32_apply(op, u)
    ref = A.apply(u)
    assert _relerr(got, ref) < 1e-5
    if bc:  # Dirichlet rows: y = x (in float)
        m = bcm.astype(bool)
        assert np.array_equal(got[m], u[m].astype(np.float32).astype(np.float64))
    got2 = _fp32_apply(op, u)  # a second application: nothing of the previous output survives
    assert _relerr(got2, ref) < 1e-5


def _fp32_hierarchy(pm, n, orders, k=3):
    from oracle import pmg_oracle as po

    h = pm.PoissonHierarchy(n, orders, kappa=2.0, cheb_its=k, warp=warp)
    mesh, ops, sm, it, mg, b, eigs = po.build_hierarchy(n, orders, cheb_its=k, warp=warp)
    for s_, e in zip(sm, h.eig_ranges):
        s_.eig_range = e
    return h, ops, mg, b


def _vec(pm, layout, a):
    v = pm.Vector(layout)
    v.data.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    return v


@pytest.mark.parametrize("orders,n", [((1, 2, 4), 4), ((1, 3, 6), 3)])
def test_fp32_vcycle_against_fp64_oracle(pm, orders, n):
    h, ops, mg, b = _fp32_hierarchy(pm, n, orders)
    h.mg.set_precision("fp32")
    assert h.mg.precision == "fp32"
    r = np.random.default_rng(11).standard_normal(b.size)
    x = h.new_vector()
    x.set(0.0)
    h.mg.apply(_vec(pm, h.layouts[-1], r), x)
    ref = mg.apply(r, np.zeros_like(r))
    assert _relerr(x.data_copy(), ref) < 1e-4
    assert all(c > 0 for c in h.mg.apply_counts())  # the stiffness launches are still counted


def _pcg(pm, h, rtol, max_iter=60):
    cg = pm.CGSolver(h.layouts[-1])
    cg.set_max_iterations(max_iter)
    cg.set_tolerance(rtol)
    x = h.new_vector()
    x.set(0.0)
    its = cg.solve(h.operators[-1], x, h.rhs[-1], preconditioner=h.mg)
    r = pm.Vector(h.layouts[-1])
    h.operators[-1](x, r)
    pm.axpy(r, -1.0, r, h.rhs[-1])
    return its, pm.norm(r) / pm.norm(h.rhs[-1])


@pytest.mark.parametrize("coarse", [None, "amg"])
def test_pcg_with_fp32_cycle(pm, coarse):
    h = pm.PoissonHierarchy(6, (1, 2, 4), kappa=2.0, cheb_its=3, warp=warp)
    amg = pm.AmgSolver(h.operators[0], cycles=2) if coarse else None  # stationary: a fixed linear preconditioner
    h.mg.set_coarse_solver(amg)
    its64, res64 = _pcg(pm, h, 1e-8)
    h.mg.set_precision("fp32")
    its32, res32 = _pcg(pm, h, 1e-8)
    assert its32 <= its64 + 1, (its32, its64)
    assert res32 < 1e-7, res32
    its32b, res32b = _pcg(pm, h, 1e-10)  # no float floor
    assert its32b < 60 and res32b < 1e-9, (its32b, res32b)


def test_fp32_defect_correction(pm):
    h = pm.PoissonHierarchy(6, (1, 2, 4), kappa=2.0, cheb_its=3, warp=warp)
    h.mg.set_coarse_solver(pm.AmgSolver(h.operators[0]))
    b = h.rhs[-1]
    bn = pm.norm(b)

    def stationary(limit):
        x = h.new_vector()
        x.set(0.0)
        for c in range(1, limit + 1):
            rn = h.mg.apply(b, x, verbose=True)
            if rn < 1e-10 * bn:
                return c, rn
        return limit + 1, rn

    c64, _ = stationary(40)
    assert c64 <= 40
    h.mg.set_precision("fp32")
    c32, rn32 = stationary(c64 + 2)
    assert c32 <= c64 + 2 and rn32 < 1e-10 * bn, (c32, c64, rn32 / bn)
    # one cycle from a non-zero initial guess against the FP64 cycle
    x0 = np.random.default_rng(5).standard_normal(b.data.numel())
    outs = {}
    for prec in ("fp64", "fp32"):
        h.mg.set_precision(prec)
        x = _vec(pm, h.layouts[-1], x0)
        h.mg.apply(b, x)
        outs[prec] = x.data_copy()
    assert _relerr(outs["fp32"], outs["fp64"]) < 1e-4


def test_fp32_lifecycle(pm):
    h = pm.PoissonHierarchy(6, (1, 2, 4), kappa=2.0, cheb_its=3, warp=warp)
    b = h.rhs[-1]
    assert h.mg.precision == "fp64"

    def cycle():
        x = h.new_vector()
        x.set(0.0)
        h.mg.apply(b, x)
        return x.data_copy()

    ref64 = cycle()
    h.mg.set_precision("fp32")
    eager32 = cycle()
    h.mg.set_graph(True)
    n0 = h.mg.graph_replays()
    graph32 = cycle()
    assert h.mg.graph_replays() > n0
    assert _relerr(graph32, eager32) < 1e-6
    h.mg.set_graph(False)
    # back to FP64: the FP64 cycle again (to its own rounding: the LDS and atomic sums meet in arrival order)
    h.mg.set_precision("fp64")
    again64 = cycle()
    assert _relerr(again64, ref64) < 1e-13
    assert _relerr(eager32, ref64) > 1e-12  # ... and FP32 really was a different computation
    h.mg.set_precision("fp32")
    assert _relerr(cycle(), eager32) < 1e-6
    # a replaced diagonal reaches the next FP32 cycle
    op = h.operators[-1]
    d = pm.Vector(h.layouts[-1])
    op.get_diag_inverse(d)
    d_half = _vec(pm, h.layouts[-1], 0.5 * d.data_copy())
    op.set_diag_inverse(d_half)
    changed = cycle()
    assert _relerr(changed, eager32) > 1e-3
    op.set_diag_inverse(d)
    assert _relerr(cycle(), eager32) < 1e-6


def test_fp32_refusals(pm):
    from pmg_dolfinx_amd import _lib

    layout = pm.Layout(10, num_ghosts=2)
    mg = pm.MultigridPreconditioner([layout], np.zeros(12, dtype=np.int8))
    with pytest.raises(_lib.PmgError, match="single-domain"):
        mg.set_precision("fp32")
    assert mg.precision == "fp64"
    with pytest.raises(_lib.PmgError, match="unknown precision"):
        _lib.call("pmg_multigrid_set_precision", mg.handle, 7)
    with pytest.raises(ValueError):
        mg.set_precision("fp16")


def _run(*args):
    path = os.path.join(BIN, "pmg_main")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_driver_fp32_cycle(built):
    args = ("--n", 24, "--orders", "1,2,4", "--amg", "--pcg", "--random-rhs", "--cycles", 2)
    pat = r"PCG with V-cycle preconditioner: (\d+) iterations, \|b - A x\| / \|b\| = (\S+),"
    r64 = _run(*args)
    assert r64.returncode == 0, r64.stdout + r64.stderr
    r32 = _run(*args, "--fp32-cycle")
    assert r32.returncode == 0, r32.stdout + r32.stderr
    assert "Cycle precision: fp32" in r32.stdout and "Cycle precision" not in r64.stdout
    (its64, _), = re.findall(pat, r64.stdout)
    (its32, res32), = re.findall(pat, r32.stdout)
    assert int(its32) <= int(its64) + 1
    assert float(res32) < 1e-6
    bad = _run("--n", 8, "--orders", "1,2", "--fp32-cycle", "--ranks", "2,1,1")
    assert bad.returncode != 0 and "single-domain" in bad.stderr
