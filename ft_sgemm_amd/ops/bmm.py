"""A fault-tolerant batched matrix product on the strided-batched ragged
fused-ABFT SGEMM.

ft_bmm(x, y) computes out = x @ y like torch.bmm, for fp32 CUDA tensors, with
the forward product and both backward products on
ops.ft_sgemm_ragged_batched: one launch per product for the whole batch,
in-kernel verify, locate and correct, and no operand copy for the layouts a
transformer block produces (head views of a projection output, transposed
keys).

In the kernels' terms (per entry c (N, M) = b(K, N)^T @ a(K, M), transposed
operands given as (M, K) / (N, K)) with row-major x (B, P, Q), y (B, Q, R)
and g = grad_out (B, P, R):

    out    (B, P, R) : a = y,           b = x (trans_b), K = Q
    grad_x (B, P, Q) : a = y (trans_a), b = g (trans_b), K = R
    grad_y (B, Q, R) : a = g,           b = x,           K = P

An operand whose unit stride lies on its second-to-last dimension (a
k.transpose(1, 2) view) is read in place as the transposed view with the
flag flipped.
"""

from __future__ import annotations

import torch

from .fault_report import BatchedFaultReport


def _check(x, y):
    """Shape and dtype rules of ft_bmm; touches no extension.  Returns the
    leading (batch) dimensions of the result."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"ft_bmm: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"ft_bmm: {name} must be float32, got {t.dtype}")
        if t.dim() < 2:
            raise ValueError(f"ft_bmm: {name} must be at least 2-D, got "
                             f"{tuple(t.shape)}")
    if x.dim() == 2 and y.dim() == 2:
        raise ValueError("ft_bmm: x and y are both 2-D: there is no batch "
                         "(use ft_linear or ft_sgemm_ragged)")
    if x.shape[-1] != y.shape[-2]:
        raise ValueError(f"ft_bmm: x {tuple(x.shape)} and y {tuple(y.shape)} "
                         f"disagree on the inner dimension")
    if x.dim() > 2 and y.dim() > 2 and x.shape[:-2] != y.shape[:-2]:
        raise ValueError(f"ft_bmm: batch dimensions {tuple(x.shape[:-2])} of "
                         f"x and {tuple(y.shape[:-2])} of y differ (no "
                         f"broadcasting; a 2-D operand is shared)")
    if x.numel() == 0 or y.numel() == 0:
        raise ValueError("ft_bmm: empty x or y")
    return tuple(x.shape[:-2] if x.dim() > 2 else y.shape[:-2])


def _in_place(t: torch.Tensor) -> bool:
    """May the ragged kernel read t's last two dimensions as they lie: unit
    inner stride, rows that do not overlap."""
    rows, width = t.shape[-2:]
    return ((width == 1 or t.stride(-1) == 1) and
            (rows == 1 or t.stride(-2) >= width))


def _operand(t: torch.Tensor, trans: bool):
    """(tensor, flag) that reads the 2-D or 3-D t, meant with transpose flag
    `trans`, without a copy where its layout allows: as it lies, or as its
    transposed view with the flag flipped.  Anything else is copied."""
    if t.dim() > 3:
        t = t.reshape(-1, *t.shape[-2:])  # a view whenever the strides allow
    if _in_place(t):
        return t, trans
    tt = t.transpose(-1, -2)
    if _in_place(tt):
        return tt, not trans
    return t.contiguous(), trans


def _product(a, trans_a, b, trans_b, c, inject, report, tier):
    from . import (choose_tier_ragged_batched, ft_sgemm_ragged_batched,
                   ragged_batched_layout)
    batch, m, n, k = ragged_batched_layout(a, b, c, trans_a, trans_b)[:4]
    ft_sgemm_ragged_batched(
        tier or choose_tier_ragged_batched(m, n, k, batch), a, b, c, 1.0, 0.0,
        inject=inject, report=report, trans_a=trans_a, trans_b=trans_b)
    return c


class _FTBmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, lead, inject, report, tier):
        batch = 1
        for d in lead:
            batch *= d
        p, r = x.shape[-2], y.shape[-1]
        out = torch.empty((batch, p, r), dtype=x.dtype, device=x.device)
        a, ta = _operand(y, False)
        b, tb = _operand(x, True)
        _product(a, ta, b, tb, out, inject, report, tier)
        ctx.save_for_backward(x, y)
        ctx.cfg = (batch, inject, report, tier)
        return out.view(*lead, p, r)

    @staticmethod
    def backward(ctx, grad_out):
        x, y = ctx.saved_tensors
        batch, inject, report, tier = ctx.cfg
        p, q, r = x.shape[-2], x.shape[-1], y.shape[-1]
        g = grad_out.reshape(batch, p, r)
        grad_x = grad_y = None
        if ctx.needs_input_grad[0]:
            a, ta = _operand(y, True)
            b, tb = _operand(g, True)
            gx = torch.empty((batch, p, q), dtype=x.dtype, device=x.device)
            _product(a, ta, b, tb, gx, inject, report, tier)
            grad_x = gx.sum(dim=0) if x.dim() == 2 else gx.view(x.shape)
        if ctx.needs_input_grad[1]:
            a, ta = _operand(g, False)
            b, tb = _operand(x, False)
            gy = torch.empty((batch, q, r), dtype=x.dtype, device=x.device)
            _product(a, ta, b, tb, gy, inject, report, tier)
            grad_y = gy.sum(dim=0) if y.dim() == 2 else gy.view(y.shape)
        return grad_x, grad_y, None, None, None, None


def ft_bmm(x: torch.Tensor, y: torch.Tensor, *, inject: bool = False,
           report: BatchedFaultReport | None = None,
           tier: str | None = None) -> torch.Tensor:
    """out = x @ y on the fused-ABFT strided-batched ragged SGEMM,
    differentiable.

    x (B, P, Q) and y (B, Q, R): fp32 CUDA tensors; out is (B, P, R).  More
    than one leading dimension (equal in x and y) is flattened with reshape.
    A 2-D x (P, Q) or y (Q, R) is shared by the whole batch; its gradient is
    the sum of the per-entry gradients over the batch, taken with a plain
    torch sum, which is NOT covered by ABFT.

    The forward product and the two backward products (grad_x = g @ y^T,
    grad_y = x^T @ g) each run one ft_sgemm_ragged_batched launch pair; only
    the gradients autograd asks for are computed.  No operand is copied when
    its unit stride lies on either of its last two dimensions and its rows do
    not overlap: head views (H, T, D) of a (T, H, D) tensor, expand()ed
    operands and k.transpose(1, 2) views are read in place, the last by
    flipping the kernel's transpose flag.  An operand is copied (contiguous())
    only when neither of its last two dimensions has stride 1, when its rows
    overlap, or when several leading dimensions do not flatten to one batch
    stride; the incoming gradient is treated the same way.

    inject: run the kernels' injector self-test in every product.
    report: one BatchedFaultReport of B entries (the flattened batch) that
    accumulates over all products.
    tier: a tier name for every product; None picks
    choose_tier_ragged_batched(m, n, k, B) per product."""
    lead = _check(x, y)
    return _FTBmmFn.apply(x, y, lead, inject, report, tier)
