"""A differentiable solve: ``x = A(kappa)^-1 b`` with gradients with respect to ``b`` and to the per-cell coefficient.

The operator is symmetric and, with the library's boundary treatment, the identity on marked rows, so the adjoint
system is the forward one: one more solve with the same operator, solver and preconditioner gives
``lambda = A^-1 dJ/dx``; then ``dJ/db = lambda`` and ``dJ/dkappa_c = -lambda^T (dA/dkappa_c) x``, which is the
per-cell bilinear form ``-e_c(x, lambda)`` of ``MatFreeLaplacian.cell_form`` (no kappa, constrained).  Not in the
reference.  Single domain only: a reverse accumulation across ranks is not provided.
"""
from __future__ import annotations

from .vector import Vector


def _as_vector(layout, t):
    import torch

    if isinstance(t, Vector):
        t = t.data
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise TypeError("a right-hand side must be a Vector or a float64 torch tensor")
    if t.numel() != layout.total:
        raise ValueError(f"the vector has {t.numel()} entries, the layout {layout.total}")
    v = Vector(layout)
    v.data.copy_(t.detach().reshape(-1))
    return v


def _solve(op, cg, pre, rhs):
    x = Vector(op.layout)  # (zeros: the guess)
    cg.solve(op, x, rhs, preconditioner=pre)
    return x.data


def _function():
    import torch

    class Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, b, kappa, op, cg, pre):
            if kappa is not op.kappa:
                if tuple(kappa.shape) != tuple(op.kappa.shape) or kappa.dtype != op.kappa.dtype:
                    raise ValueError(f"kappa must be a float64 tensor of shape {tuple(op.kappa.shape)}")
                with torch.no_grad():
                    op.kappa.copy_(kappa)
            op.compute_diag_inverse()
            x = _solve(op, cg, pre, _as_vector(op.layout, b))
            ctx.op, ctx.cg, ctx.pre = op, cg, pre
            ctx.kappa_version = op.kappa._version
            ctx.x = x.clone()  # the caller may write into what it gets
            return x

        @staticmethod
        def backward(ctx, grad_x):
            op = ctx.op
            if op.kappa._version != ctx.kappa_version:
                raise RuntimeError("adjoint.solve: the operator's kappa was modified between forward and backward; "
                                   "the adjoint solve would use another operator than the forward one")
            lam = _solve(op, ctx.cg, ctx.pre, _as_vector(op.layout, grad_x.contiguous()))
            grad_b = lam if ctx.needs_input_grad[0] else None
            grad_kappa = -op.cell_form(ctx.x, lam, kappa=False, constrained=True) if ctx.needs_input_grad[1] else None
            return grad_b, grad_kappa, None, None, None

    return Solve


_Solve = None


def solve(op, cg, b, kappa, preconditioner=None):
    """``x = A(kappa)^-1 b`` by ``cg.solve`` from a zero guess, differentiable in ``b`` and ``kappa``.

    ``op`` is a ``MatFreeLaplacian`` on a single-domain layout, ``cg`` a ``CGSolver`` (its tolerance bounds the accuracy
    of both the solution and the gradients), ``b`` a float64 device tensor of the layout's size (or a ``Vector``),
    ``kappa`` a float64 device tensor ``[ncells]``: the operator's own ``op.kappa``, or another tensor, which is copied
    into ``op.kappa`` in place.  ``op.compute_diag_inverse()`` runs before the solve.  A multigrid ``preconditioner`` is
    used as given: its smoother bounds and an AMG renewal after a change of kappa stay the caller's business.  Returns
    the solution as a tensor of the layout's size.  Backward is one more solve with the same three objects; it raises if
    ``op.kappa`` was modified in place since the forward solve."""
    global _Solve
    import torch

    layout = op.layout
    if layout.num_ghosts > 0 or layout.distributed:
        raise ValueError("adjoint.solve: single domain only (the layout has ghosts or a communicator); the reverse "
                         "accumulation across ranks is not provided")
    if not isinstance(kappa, torch.Tensor):
        raise TypeError("kappa must be a float64 torch tensor: op.kappa or one of its shape")
    if isinstance(b, Vector):
        b = b.data
    if _Solve is None:
        _Solve = _function()
    return _Solve.apply(b, kappa, op, cg, preconditioner)
