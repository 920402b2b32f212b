"""The differentiable solve with every coefficient (pmg_dolfinx_amd.adjoint.solve, keywords field / tensor / sigma):
gradients of J = g . x, x = A^-1 b, with respect to b, kappa, the nodal field, the per-cell tensor and the reaction
coefficient from ONE backward, against dense numpy on the oracle's operator.

Set-up, as tests/test_gpu_adjoint.py: a jittered 2x2x2 box at degree 2 (125 dofs, 8 cells), Dirichlet on the face x = 0
with non-zero b there, CG tolerance 1e-12, preconditioned by Jacobi and by the (1, 2) multigrid; a random field in
[1, 2], random symmetric positive-definite tensors, sigma in [0, 3], kappa in [1, 2].  The multigrid's coarse level gets
the per-cell coefficients too and both smoothers their bounds anew, so that it is the preconditioner of this operator.

Truth: x and lambda from dense solves; A is linear in each coefficient, so dJ/dp = -lambda . (A(p + d e) x - A(p) x) / d
exactly, with the oracle's operator (an O(1) step; 0.25 for an off-diagonal tensor entry, which keeps the tensor
positive definite).

Bar, that file's, measured in the test: err = max(relative max-norm error of the library's x and of its
lambda = A^-1 g against the dense solves, 1e-14), both from the existing CG, called directly.  Every gradient is bilinear
in (x, lambda) and inherits exactly that error: it must agree within 100 * err relative to its own max norm."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cell_form_reference as cf  # noqa: E402
import curved_geometry_reference as cr  # noqa: E402
import reaction_reference as rr  # noqa: E402
import tensor_coefficient_reference as tr  # noqa: E402
from oracle import pmg_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P, N = 2, 2
NAMES = ("kappa", "field", "tensor", "sigma")


@pytest.fixture(scope="module")
def pm(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


class Problem:
    def __init__(self, pm):
        self.pm = pm
        # (the face x = 0 moves by the jitter, at most 0.03; the next plane of dofs is at 0.25)
        self.h = h = pm.PoissonHierarchy(N, (1, P), kappa=2.0, warp=cf.jitter, dirichlet=lambda x: x[:, 0] < 0.1)
        self.op, self.layout, self.lv = h.operators[-1], h.layouts[-1], h.levels[-1]
        assert self.lv.ndofs == 125 and h.part.ncells == 8 and self.op.kappa is h.kappa
        rng = np.random.default_rng(43)
        self.p = {"kappa": rng.uniform(1.0, 2.0, 8), "field": rng.uniform(1.0, 2.0, 125),
                  "tensor": tr.random_spd(8, 11), "sigma": rng.uniform(0.0, 3.0, 8)}
        self.b_h, self.g_h = rng.standard_normal(125), rng.standard_normal(125)
        self.cg = pm.CGSolver(self.layout)
        self.cg.set_max_iterations(500)
        self.cg.set_tolerance(1e-12)

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    def install(self):
        """The coefficients on the fine operator, the per-cell ones (and the field's mean) on the coarse one; the
        levels' inverse diagonals and smoother bounds follow."""
        h, pm = self.h, self.pm
        with torch.no_grad():
            h.kappa.copy_(self.dev(self.p["kappa"]))
        for op, layout in zip(h.operators, h.layouts):
            kq = pm.Vector(layout)
            if op is self.op:
                kq.data.copy_(self.dev(self.p["field"]))
            else:
                kq.set(1.5)
            op.set_coefficient_field(kq)
            op.set_coefficient_tensor(self.p["tensor"])
            op.set_reaction(self.p["sigma"])
            op.compute_diag_inverse()
        smoothers = []
        for op, layout in zip(h.operators, h.layouts):  # as PoissonHierarchy estimates them
            cg = pm.CGSolver(layout)
            cg.set_max_iterations(20)
            cg.set_tolerance(1e-6)
            cg.store_coefficients(True)
            x, y = pm.Vector(layout), pm.Vector(layout)
            x.set(0.0)
            y.set(1.0)
            cg.solve(op, x, y)
            top = np.sort(cg.compute_eigenvalues())[-1]
            sm = pm.Chebyshev(layout, (0.1 * top, 1.1 * top))
            sm.set_max_iterations(3)
            smoothers.append(sm)
        h.smoothers = smoothers
        h.mg.set_solvers(smoothers)

    def operator(self, **changed):
        """The oracle's operator with the problem's coefficients, some of them replaced."""
        p = {**self.p, **changed}
        h = self.h
        A = cr.laplacian(P, 1, p["kappa"], self.lv.dofmap, h.part.xgeom, h.part.geom_dofmap, self.lv.bc_marker)
        return rr.ReactionLaplacian(cr.with_tensor(A, p["tensor"], p["field"]), p["sigma"], h.part.xgeom,
                                    h.part.geom_dofmap)

    def truth(self):
        A = self.operator().dense()
        x, lam = np.linalg.solve(A, self.b_h), np.linalg.solve(A.T, self.g_h)
        y0 = self.operator().apply(x)
        assert np.abs(y0 - A @ x).max() <= 1e-12 * np.abs(y0).max()  # the operator that is stepped is the dense one
        grads = {}
        for name in NAMES:
            out = np.empty(self.p[name].shape)
            for idx in np.ndindex(out.shape):
                step = 0.25 if name == "tensor" and idx[1] in (1, 2, 4) else 1.0
                p1 = self.p[name].copy()
                p1[idx] += step
                out[idx] = -lam @ (self.operator(**{name: p1}).apply(x) - y0) / step
            grads[name] = out
        return x, lam, grads

    def cg_solve(self, rhs, pre):
        x, b = self.pm.Vector(self.layout), self.pm.Vector(self.layout)
        b.data.copy_(self.dev(rhs))
        self.cg.solve(self.op, x, b, preconditioner=pre)
        return x.data_copy()

    def solver_error(self, truth, pre=None):
        """The existing solver's own error, on the two systems the gradients are made of."""
        x_t, lam_t, _ = truth
        x_cg, lam_cg = self.cg_solve(self.b_h, pre), self.cg_solve(self.g_h, pre)
        return max(np.abs(x_cg - x_t).max() / np.abs(x_t).max(), np.abs(lam_cg - lam_t).max() / np.abs(lam_t).max(),
                   1e-14)

    def field_vector(self):
        kq = self.pm.Vector(self.layout)
        kq.data.copy_(self.dev(self.p["field"]))
        return kq

    def tensors(self, *names):
        """Leaf tensors of the coefficients; those named require a gradient."""
        return {k: self.dev(v).requires_grad_(k in names) for k, v in self.p.items()}


@pytest.fixture(scope="module")
def problem(pm):
    pr = Problem(pm)
    pr.install()
    return pr


@pytest.fixture(scope="module")
def truth(problem):
    return problem.truth()


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
def test_one_backward_gives_every_gradient(problem, truth, precond):
    pr = problem
    x_t, lam_t, grads_t = truth
    pre = pr.h.mg if precond == "multigrid" else None
    err = pr.solver_error(truth, pre)
    b = pr.dev(pr.b_h).requires_grad_(True)
    g = pr.dev(pr.g_h)
    t = pr.tensors(*NAMES)
    calls = []
    original = pr.op.form_gradients
    pr.op.form_gradients = lambda *a, **kw: (calls.append(kw), original(*a, **kw))[1]
    try:
        x = pr.pm.adjoint.solve(pr.op, pr.cg, b, t["kappa"], preconditioner=pre, field=t["field"], tensor=t["tensor"],
                                sigma=t["sigma"])
        J = (g * x).sum()
        got = torch.autograd.grad(J, (b,) + tuple(t[k] for k in NAMES))
    finally:
        del pr.op.form_gradients
    assert calls == [dict(constrained=True, kappa=True, field=True, tensor=True, sigma=True)]  # one call
    ex = np.abs(x.detach().cpu().numpy() - x_t).max() / np.abs(x_t).max()
    eb = np.abs(got[0].cpu().numpy() - lam_t).max() / np.abs(lam_t).max()
    print(f"{precond}: err (x, lambda of the CG) = {err:.3e}, bar {100 * err:.3e}; x {ex:.3e}, dJ/db {eb:.3e}")
    assert ex <= 100 * err and eb <= 100 * err
    for name, grad in zip(NAMES, got[1:]):
        want = grads_t[name]
        assert tuple(grad.shape) == want.shape
        e = np.abs(grad.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"{precond}: dJ/d{name} {e:.3e}")
        assert e <= 100 * err, name


def test_a_subset_of_keywords_gives_gradients_for_those_only(problem, truth):
    pr = problem
    _, _, grads_t = truth
    err = pr.solver_error(truth)
    t = pr.tensors("sigma")  # the field is given, without a gradient; the tensor stays as the operator has it
    b = pr.dev(pr.b_h)
    calls = []
    original = pr.op.form_gradients
    pr.op.form_gradients = lambda *a, **kw: (calls.append(kw), original(*a, **kw))[1]
    try:
        x = pr.pm.adjoint.solve(pr.op, pr.cg, b, pr.op.kappa, field=t["field"], sigma=t["sigma"])
        (pr.dev(pr.g_h) * x).sum().backward()
    finally:
        del pr.op.form_gradients
    assert calls == [dict(constrained=True, kappa=False, field=False, tensor=False, sigma=True)]
    assert t["field"].grad is None and b.grad is None and pr.op.kappa.grad is None
    want = grads_t["sigma"]
    assert np.abs(t["sigma"].grad.cpu().numpy() - want).max() <= 100 * err * np.abs(want).max()


def test_setting_a_coefficient_between_forward_and_backward_raises(problem):
    pr = problem
    t = pr.tensors("field")
    x = pr.pm.adjoint.solve(pr.op, pr.cg, pr.dev(pr.b_h), pr.op.kappa, field=t["field"])
    epoch = pr.op.coefficient_epoch
    pr.op.set_reaction(pr.p["sigma"])  # the same values: the guard counts calls, it does not compare
    assert pr.op.coefficient_epoch == epoch + 1
    with pytest.raises(RuntimeError, match="between forward and backward"):
        x.sum().backward()
    assert t["field"].grad is None
    # every setter counts
    fc, fl = pr.h.part.exterior_facets()
    for change in (lambda: pr.op.set_coefficient_tensor(pr.p["tensor"]), lambda: pr.op.set_robin(fc[:0], fl[:0], None),
                   lambda: pr.op.set_coefficient_field(pr.field_vector())):
        epoch = pr.op.coefficient_epoch
        change()
        assert pr.op.coefficient_epoch == epoch + 1


def test_a_non_positive_field_is_refused_with_the_operator_unchanged(problem):
    pr = problem
    x_v, y0, y1 = pr.pm.Vector(pr.layout), pr.pm.Vector(pr.layout), pr.pm.Vector(pr.layout)
    x_v.data.copy_(pr.dev(pr.g_h))
    pr.op(x_v, y0)
    kappa_before, tensor_before = pr.op.kappa.clone(), pr.op.geometry()  # (G: the field and the tensor are in it)
    bad = pr.p["field"].copy()
    bad[17] = -1.0
    with pytest.raises(pr.pm._lib.PmgError, match="pmg_laplacian_set_coefficient_field"):
        pr.pm.adjoint.solve(pr.op, pr.cg, pr.dev(pr.b_h), pr.dev(pr.p["kappa"][::-1].copy()), field=pr.dev(bad),
                            sigma=pr.dev(np.zeros(8)))
    pr.op(x_v, y1)
    assert torch.equal(pr.op.geometry(), tensor_before) and torch.equal(pr.op.kappa, kappa_before)
    # (an apply of a mesh this small adds with atomics: two of them agree to rounding, the project's 1e-12, not in bytes)
    assert float((y1.data - y0.data).abs().max()) <= 1e-12 * float(y0.data.abs().max())
    assert pr.op.has_coefficient_field() and pr.op.has_reaction()
    with pytest.raises(ValueError):
        pr.pm.adjoint.solve(pr.op, pr.cg, pr.dev(pr.b_h), pr.op.kappa, tensor=pr.dev(pr.p["tensor"][:, :5]))
    with pytest.raises(TypeError):
        pr.pm.adjoint.solve(pr.op, pr.cg, pr.dev(pr.b_h), pr.op.kappa, sigma=pr.p["sigma"])


def test_the_old_signature_still_returns_the_kappa_gradient(pm):
    """tests/test_gpu_adjoint.py's case on a fresh hierarchy, called without the new keywords: no coefficient is set,
    and the gradient is that file's dense one within that file's bar."""
    pr = Problem(pm)
    kappa_h = pr.p["kappa"]
    dense = lambda k: po.Laplacian(P, k, pr.lv.dofmap, pr.h.part.xgeom, pr.h.part.geom_dofmap,  # noqa: E731
                                   pr.lv.bc_marker).assemble_csr().toarray()
    A = dense(kappa_h)
    x_t, lam_t = np.linalg.solve(A, pr.b_h), np.linalg.solve(A.T, pr.g_h)
    dk_t = np.empty(8)
    for c in range(8):
        k1 = kappa_h.copy()
        k1[c] += 1.0
        dk_t[c] = -lam_t @ ((dense(k1) - A) @ x_t)
    with torch.no_grad():
        pr.h.kappa.copy_(pr.dev(kappa_h))
    pr.op.compute_diag_inverse()
    x_cg, lam_cg = pr.cg_solve(pr.b_h, None), pr.cg_solve(pr.g_h, None)
    err = max(np.abs(x_cg - x_t).max() / np.abs(x_t).max(), np.abs(lam_cg - lam_t).max() / np.abs(lam_t).max(), 1e-14)
    b = pr.dev(pr.b_h).requires_grad_(True)
    kappa = pr.dev(kappa_h).requires_grad_(True)
    epoch = pr.op.coefficient_epoch
    x = pm.adjoint.solve(pr.op, pr.cg, b, kappa)
    grad_b, grad_k = torch.autograd.grad((pr.dev(pr.g_h) * x).sum(), (b, kappa))
    assert pr.op.coefficient_epoch == epoch
    assert not (pr.op.has_coefficient_field() or pr.op.has_coefficient_tensor() or pr.op.has_reaction())
    assert np.abs(grad_b.cpu().numpy() - lam_t).max() <= 100 * err * np.abs(lam_t).max()
    assert np.abs(grad_k.cpu().numpy() - dk_t).max() <= 100 * err * np.abs(dk_t).max()
