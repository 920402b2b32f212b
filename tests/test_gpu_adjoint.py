"""The differentiable solve (pmg_dolfinx_amd.adjoint.solve): gradients of J = g . x, x = A(kappa)^-1 b, with respect to b
and to the per-cell coefficient, against dense numpy on the oracle's assembled matrix.

Set-up: a jittered 2x2x2 box at degree 2 (125 dofs, 8 cells), Dirichlet on the face x = 0 with non-zero b there, kappa
random in [1, 2], CG tolerance 1e-12, preconditioned by Jacobi and by the (1, 2) multigrid.

Bar, measured in the test: err = max(relative max-norm error of the library's x and of its lambda = A^-1 g against the
dense solves, 1e-14) -- both from the existing CG, called directly.  The gradient is bilinear in (x, lambda), so it
inherits their errors; the gradients must agree within 100 * err relative to max_c |dJ/dkappa_c| and to max |lambda|
(the factor covers the ratio between the max norm and the cell energy norms on eight cells)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cell_form_reference as cf  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P, N = 2, 2


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


class Problem:
    def __init__(self, pm):
        # (the face x = 0 moves by the jitter, at most 0.03; the next plane of dofs is at 0.25)
        self.h = h = pm.PoissonHierarchy(N, (1, P), kappa=2.0, warp=cf.jitter, dirichlet=lambda x: x[:, 0] < 0.1)
        self.op, self.layout, self.lv = h.operators[-1], h.layouts[-1], h.levels[-1]
        assert self.lv.ndofs == 125 and h.part.ncells == 8 and self.op.kappa is h.kappa
        rng = np.random.default_rng(42)
        self.kappa_h = rng.uniform(1.0, 2.0, 8)
        self.b_h = rng.standard_normal(125)  # non-zero on the marked rows too
        self.g_h = rng.standard_normal(125)
        self.cg = pm.CGSolver(self.layout)
        self.cg.set_max_iterations(500)
        self.cg.set_tolerance(1e-12)
        self.pm = pm

    def set_kappa(self, values):
        """Every level shares the one coefficient array; the levels' inverse diagonals follow (the smoother bounds stay
        those of kappa = 2, which bounds every value here from above)."""
        with torch.no_grad():
            self.h.kappa.copy_(torch.from_numpy(np.ascontiguousarray(values)).cuda())
        for op in self.h.operators:
            op.compute_diag_inverse()

    def dense(self, kappa):
        h = self.h
        A = po.Laplacian(P, kappa, self.lv.dofmap, h.part.xgeom, h.part.geom_dofmap, self.lv.bc_marker)
        return A.assemble_csr().toarray()

    def truth(self):
        A = self.dense(self.kappa_h)
        x, lam = np.linalg.solve(A, self.b_h), np.linalg.solve(A.T, self.g_h)
        dk = np.empty(8)
        for c in range(8):
            k1 = self.kappa_h.copy()
            k1[c] += 1.0
            dk[c] = -lam @ ((self.dense(k1) - A) @ x)
        return x, lam, dk

    def cg_solve(self, rhs, pre):
        x, b = self.pm.Vector(self.layout), self.pm.Vector(self.layout)
        b.data.copy_(torch.from_numpy(rhs).cuda())
        self.cg.solve(self.op, x, b, preconditioner=pre)
        return x.data_copy()


@pytest.fixture(scope="module")
def problem(pm):
    return Problem(pm)


@pytest.fixture(scope="module")
def truth(problem):
    return problem.truth()


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
def test_autograd_matches_the_dense_adjoint(problem, truth, precond):
    pr = problem
    x_t, lam_t, dk_t = truth
    pre = pr.h.mg if precond == "multigrid" else None
    pr.set_kappa(pr.kappa_h)
    # the existing solver's own error, on the two systems the gradient is made of
    x_cg, lam_cg = pr.cg_solve(pr.b_h, pre), pr.cg_solve(pr.g_h, pre)
    err = max(np.abs(x_cg - x_t).max() / np.abs(x_t).max(), np.abs(lam_cg - lam_t).max() / np.abs(lam_t).max(), 1e-14)
    b = torch.from_numpy(pr.b_h).cuda().requires_grad_(True)
    g = torch.from_numpy(pr.g_h).cuda()
    if precond == "jacobi":  # a tensor of the caller's: copied into the operator's
        pr.set_kappa(np.full(8, 2.0))
        kappa = torch.from_numpy(pr.kappa_h).cuda().requires_grad_(True)
    else:  # the operator's own
        kappa = pr.op.kappa.requires_grad_(True)
    try:
        x = pr.pm.adjoint.solve(pr.op, pr.cg, b, kappa, preconditioner=pre)
        assert torch.equal(pr.op.kappa.detach(), torch.from_numpy(pr.kappa_h).cuda())
        J = (g * x).sum()
        grad_b, grad_k = torch.autograd.grad(J, (b, kappa))
    finally:
        pr.op.kappa.requires_grad_(False)
    ex = np.abs(x.detach().cpu().numpy() - x_t).max() / np.abs(x_t).max()
    eb = np.abs(grad_b.cpu().numpy() - lam_t).max() / np.abs(lam_t).max()
    ek = np.abs(grad_k.cpu().numpy() - dk_t).max() / np.abs(dk_t).max()
    print(f"{precond}: err (x, lambda of the CG) = {err:.3e}; x {ex:.3e}, dJ/db {eb:.3e}, dJ/dkappa {ek:.3e}; "
          f"bar {100 * err:.3e}")
    assert grad_k.shape == (8,) and grad_b.shape == (125,)
    assert ex <= 100 * err and eb <= 100 * err and ek <= 100 * err


def test_backward_after_a_change_of_kappa_raises(problem):
    pr = problem
    pr.set_kappa(pr.kappa_h)
    b = torch.from_numpy(pr.b_h).cuda().requires_grad_(True)
    kappa = torch.from_numpy(pr.kappa_h).cuda().requires_grad_(True)
    x = pr.pm.adjoint.solve(pr.op, pr.cg, b, kappa)
    with torch.no_grad():
        pr.op.kappa.mul_(1.5)  # the adjoint solve would run with another operator than the forward one
    with pytest.raises(RuntimeError, match="modified"):
        x.sum().backward()
    assert b.grad is None and kappa.grad is None


def test_separate_kappa_is_copied_into_the_operator(problem):
    pr = problem
    pr.set_kappa(np.full(8, 2.0))
    other = torch.from_numpy(pr.kappa_h[::-1].copy()).cuda()
    where = pr.op.kappa.data_ptr()
    x = pr.pm.adjoint.solve(pr.op, pr.cg, torch.from_numpy(pr.b_h).cuda(), other)
    assert pr.op.kappa.data_ptr() == where and torch.equal(pr.op.kappa, other)  # in place: the kernels read this array
    want = np.linalg.solve(pr.dense(pr.kappa_h[::-1]), pr.b_h)
    # (which array was solved with, not how well: a residual of 1e-12 and a condition number below 1e3 at 125 dofs)
    assert np.abs(x.cpu().numpy() - want).max() <= 1e-9 * np.abs(want).max()
    assert not x.requires_grad
    with pytest.raises(ValueError):
        pr.pm.adjoint.solve(pr.op, pr.cg, torch.from_numpy(pr.b_h).cuda(), other[:-1])


def test_layout_with_ghosts_is_refused(pm):
    part = pm.BoxPartition((2, 2, 4), (1, 1, 2), 0)
    lv = part.level(1)
    layout = pm.make_layout(lv)
    assert layout.num_ghosts > 0
    kappa = torch.ones(part.ncells, dtype=torch.float64, device="cuda")
    op = pm.MatFreeLaplacian(1, kappa, lv.dofmap, part.xgeom, part.geom_dofmap, lv.lcells, lv.bcells, lv.bc_marker,
                             layout)
    cg = pm.CGSolver(layout)
    b = torch.zeros(layout.total, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="single domain"):
        pm.adjoint.solve(op, cg, b, kappa)
