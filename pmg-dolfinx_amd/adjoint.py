"""A differentiable solve: ``x = A^-1 b`` with gradients with respect to ``b`` and to the operator's coefficients: the
per-cell ``kappa``, the nodal field, the per-cell tensor and the per-cell reaction coefficient.

The operator is symmetric and, with the library's boundary treatment, the identity on marked rows, so the adjoint
system is the forward one: one more solve with the same operator, solver and preconditioner gives
``lambda = A^-1 dJ/dx``; then ``dJ/db = lambda`` and, for a coefficient ``p``, ``dJ/dp = -lambda^T (dA/dp) x``: minus
the outputs of ``MatFreeLaplacian.form_gradients(x, lambda, constrained=True)``, one call for all the gradients
autograd asks for.  The kappa gradient comes from that kernel too, also in a call without the keyword coefficients: it
is ``cell_form(x, lambda, kappa=False, constrained=True)`` to rounding, not byte for byte.  Not in the reference.  Single domain only: a reverse accumulation across ranks is not provided.
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


def _coefficient(name, t, shape):
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise TypeError(f"{name} must be a float64 torch tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, the operator needs {tuple(shape)}")
    return t.detach().contiguous()


def _function():
    import torch

    class Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, b, kappa, field, tensor, sigma, op, cg, pre):
            if kappa is not op.kappa and (tuple(kappa.shape) != tuple(op.kappa.shape) or kappa.dtype != op.kappa.dtype):
                raise ValueError(f"kappa must be a float64 tensor of shape {tuple(op.kappa.shape)}")
            # the three set_* calls first, each refusing what the library refuses (the operator is then as the calls
            # before it left it), kappa last: it cannot be refused
            if field is not None:
                op.set_coefficient_field(_as_vector(op.layout, _coefficient("field", field, (op.layout.total,))))
            if tensor is not None:
                op.set_coefficient_tensor(_coefficient("tensor", tensor, (op.ncells, 6)))
            if sigma is not None:
                op.set_reaction(_coefficient("sigma", sigma, (op.ncells,)))
            if kappa is not op.kappa:
                with torch.no_grad():
                    op.kappa.copy_(kappa)
            op.compute_diag_inverse()
            x = _solve(op, cg, pre, _as_vector(op.layout, b))
            ctx.op, ctx.cg, ctx.pre = op, cg, pre
            ctx.kappa_version, ctx.epoch = op.kappa._version, op.coefficient_epoch
            ctx.x = x.clone()  # the caller may write into what it gets
            return x

        @staticmethod
        def backward(ctx, grad_x):
            op = ctx.op
            if op.kappa._version != ctx.kappa_version or op.coefficient_epoch != ctx.epoch:
                raise RuntimeError("adjoint.solve: the operator's kappa was modified, or one of its coefficients set, "
                                   "between forward and backward; the adjoint solve would use another operator than "
                                   "the forward one")
            lam = _solve(op, ctx.cg, ctx.pre, _as_vector(op.layout, grad_x.contiguous()))
            grad_b = lam if ctx.needs_input_grad[0] else None
            wanted = dict(zip(op.GRADIENTS, ctx.needs_input_grad[1:5]))
            grads = op.form_gradients(ctx.x, lam, constrained=True, **wanted) if any(wanted.values()) else {}
            return (grad_b,) + tuple(-grads[k] if k in grads else None for k in op.GRADIENTS) + (None, None, None)

    return Solve


_Solve = None


def solve(op, cg, b, kappa, preconditioner=None, *, field=None, tensor=None, sigma=None):
    """``x = A^-1 b`` by ``cg.solve`` from a zero guess, differentiable in ``b``, ``kappa`` and the coefficients given
    by keyword.

    ``op`` is a ``MatFreeLaplacian`` on a single-domain layout, ``cg`` a ``CGSolver`` (its tolerance bounds the accuracy
    of both the solution and the gradients), ``b`` a float64 device tensor of the layout's size (or a ``Vector``),
    ``kappa`` a float64 device tensor ``[ncells]``: the operator's own ``op.kappa``, or another tensor, which is copied
    into ``op.kappa`` in place.  ``field`` (the layout's total size), ``tensor`` ``[ncells, 6]`` and ``sigma``
    ``[ncells]`` are float64 device tensors installed with ``op.set_coefficient_field``, ``set_coefficient_tensor`` and
    ``set_reaction``, whose refusals (a non-positive field, ...) propagate; ``None`` leaves that coefficient as the
    operator has it, and no gradient is taken with respect to it.  ``op.compute_diag_inverse()`` runs before the solve.
    A multigrid ``preconditioner`` is used as given: its smoother bounds and an AMG renewal after a change of
    coefficient stay the caller's business.  Returns the solution as a tensor of the layout's size.  Backward is one more
    solve with the same three objects and one ``op.form_gradients`` call; it raises if ``op.kappa`` was modified in
    place, or a coefficient of the operator set (``op.coefficient_epoch``), since the forward solve."""
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
    return _Solve.apply(b, kappa, field, tensor, sigma, op, cg, preconditioner)
