"""A fault-tolerant linear layer on the ragged fused-ABFT SGEMM.

ft_linear(x, weight, bias) computes y = x @ weight^T + bias like
torch.nn.functional.linear, for fp32 CUDA tensors, with all three products of
the forward and backward pass on ops.ft_sgemm_ragged: in-kernel verify,
locate and correct, and no operand copy.  The transposed-operand forms of
the ragged kernel are what make that possible: x (tokens, in) and weight
(out, in) both have K = in as their inner dimension.

In the kernels' terms (c (N, M) = b(K, N)^T @ a(K, M), transposed operands
given as (M, K) / (N, K)):

    y      (tokens, out) : a = weight (trans_a), b = x      (trans_b), K = in
    grad_x (tokens, in)  : a = weight,           b = grad_y (trans_b), K = out
    grad_w (out, in)     : a = x,                b = grad_y,           K = tokens

grad_bias is a plain torch sum over the tokens and is NOT covered by ABFT.
"""

from __future__ import annotations

import torch
from torch import nn

from ..kernel_table import TILING
from .fault_report import FaultReport


def _check(x, weight, bias):
    """Shape and dtype rules of ft_linear; touches no extension."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"ft_linear: {name} must be float32, got "
                             f"{t.dtype}")
    if weight.dim() != 2:
        raise ValueError(f"ft_linear: weight must be (out, in), got "
                         f"{tuple(weight.shape)}")
    if x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"ft_linear: x {tuple(x.shape)} does not end in "
                         f"in_features = {weight.shape[1]}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"ft_linear: bias must be ({weight.shape[0]},), got "
                         f"{tuple(bias.shape)}")
    if x.numel() == 0 or weight.numel() == 0:
        raise ValueError("ft_linear: empty x or weight")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """t as a 2-D (rows, width) tensor the ragged kernel can read in place:
    unit inner stride, rows that do not overlap.  A copy is made only when
    the tensor does not already lie like that."""
    t2 = t.reshape(-1, t.shape[-1])  # a view whenever the strides allow one
    if t2.shape[1] != 1 and t2.stride(1) != 1:
        return t2.contiguous()
    if t2.shape[0] != 1 and t2.stride(0) < t2.shape[1]:
        return t2.contiguous()
    return t2


def _product(a, b, c, beta, trans_a, trans_b, inject, report, tier,
             streamk=False):
    from .. import ops  # the gate is looked up at call time
    m, n, k = ops.ragged_layout(a, b, c, trans_a, trans_b)[:3]
    sk = 0
    if streamk:
        # the caller's tier, or the first stream-K tier the gate opens: its
        # True says stream-K there beats the classic launch on the chosen tier
        for cand in ((tier,) if tier else ("huge", "large")):
            if TILING[cand].get("streamk", False) and \
                    ops.ragged_streamk_gate(cand, m, n, k, True):
                tier, sk = cand, "auto"
                break
    tier = tier or ops.choose_tier(m, n, k, ragged=True)
    ops.ft_sgemm_ragged(tier, a, b, c, 1.0, beta, inject=inject,
                        report=report, trans_a=trans_a, trans_b=trans_b,
                        streamk=sk)


class _FTLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, inject, report, tier, streamk):
        x2 = _rows(x)
        w = _rows(weight)
        tokens, out = x2.shape[0], w.shape[0]
        if bias is not None:
            y = bias.detach().expand(tokens, out).contiguous()
        else:
            y = torch.empty((tokens, out), dtype=x.dtype, device=x.device)
        _product(w, x2, y, 0.0 if bias is None else 1.0, True, True, inject,
                 report, tier, streamk)
        ctx.save_for_backward(x2, w)
        ctx.x_shape = x.shape
        ctx.has_bias = bias is not None
        ctx.cfg = (inject, report, tier, streamk)
        return y.view(*x.shape[:-1], out)

    @staticmethod
    def backward(ctx, grad_y):
        x2, w = ctx.saved_tensors
        inject, report, tier, streamk = ctx.cfg
        g = _rows(grad_y)
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.empty_like(x2, memory_format=torch.contiguous_format)
            _product(w, g, grad_x, 0.0, False, True, inject, report, tier,
                     streamk)
            grad_x = grad_x.view(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            grad_w = torch.empty_like(w, memory_format=torch.contiguous_format)
            _product(x2, g, grad_w, 0.0, False, False, inject, report, tier,
                     streamk)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_b = g.sum(dim=0)
        return grad_x, grad_w, grad_b, None, None, None, None


def ft_linear(x: torch.Tensor, weight: torch.Tensor,
              bias: torch.Tensor | None = None, *, inject: bool = False,
              report: FaultReport | None = None,
              tier: str | None = None, streamk: bool = False) -> torch.Tensor:
    """y = x @ weight^T + bias on the fused-ABFT ragged SGEMM, differentiable.

    x (..., in), weight (out, in), bias (out,) or None: fp32 CUDA tensors.
    x is flattened to 2-D and read in place; it is copied only if its inner
    stride is not 1 (or its leading dimensions do not flatten to one row
    stride).  With a bias, y is pre-filled with it and the product runs with
    beta = 1; without, beta = 0 on an uninitialised output.

    The forward product and the two backward products (grad_x, grad_weight)
    each run ft_sgemm_ragged, with no operand transposed in memory; only the
    gradients autograd asks for are computed.  grad_bias is a plain torch sum
    and is not ABFT-covered.

    inject: run the kernels' injector self-test in every product.
    report: one FaultReport that accumulates over all products.
    tier: a tier name for every product; None picks
    choose_tier(m, n, k, ragged=True) per product.
    streamk: let each product take the stream-K decomposition at the device
    grid where ragged_streamk_gate expects it to win (grad_weight, few tiles
    and K = tokens, is the case it is for): on `tier` when one is given,
    otherwise on the first of huge and large the gate opens for the
    product's shape, in place of the chosen tier.  False, the default, is
    the classic launch everywhere."""
    _check(x, weight, bias)
    return _FTLinearFn.apply(x, weight, bias, inject, report, tier, streamk)


class FTLinear(nn.Linear):
    """nn.Linear whose forward and backward products run on ft_linear.
    Parameters, initialisation and state_dict are nn.Linear's."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 *, inject: bool = False, report: FaultReport | None = None,
                 tier: str | None = None, streamk: bool = False,
                 device=None):
        super().__init__(in_features, out_features, bias=bias, device=device,
                         dtype=torch.float32)
        self.inject, self.report, self.tier = inject, report, tier
        self.streamk = streamk

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ft_linear(x, self.weight, self.bias, inject=self.inject,
                         report=self.report, tier=self.tier,
                         streamk=self.streamk)
