"""A fault-tolerant grouped linear layer (the expert layer of a
mixture-of-experts block) on the grouped fused-ABFT SGEMM.

ft_grouped_linear(x, weight, counts, bias) applies expert e's linear layer
weight[e] (out, in), bias[e] to its own run of rows of x: with the rows of
x (T, in) sorted by expert and counts[e] rows belonging to expert e,

    y[rows of e] = x[rows of e] @ weight[e]^T + bias[e]

The forward product and both backward products are one ops.ft_sgemm_grouped
launch each over all experts, with in-kernel verify, locate and correct and
no operand copy.  The mapping is ft_linear's (ops/linear.py), per expert, in
the kernels' terms (c (N, M) = b(K, N)^T @ a(K, M), transposed operands given
as (M, K) / (N, K)), with n_e = counts[e]:

    y_e      (n_e, out) : a = weight[e] (trans_a), b = x_e      (trans_b), K = in
    grad_x_e (n_e, in)  : a = weight[e],           b = grad_y_e (trans_b), K = out
    grad_w_e (out, in)  : a = x_e,                 b = grad_y_e,           K = n_e

An expert without tokens is an entry with N = 0 in the first two products (no
tiles) and with K = 0 in the third, which writes it an exactly zero
grad_weight.  grad_bias is a plain torch segment sum and is NOT covered by
ABFT.
"""

from __future__ import annotations

import operator

import torch

from .fault_report import BatchedFaultReport
from .linear import _rows


def _counts(counts, experts, tokens):
    """counts as a list of E non-negative Python ints summing to tokens."""
    if isinstance(counts, torch.Tensor):
        if counts.is_cuda:
            raise ValueError(
                "ft_grouped_linear: counts is a CUDA tensor; reading it "
                "would synchronise with the device.  Pass counts.cpu() (or "
                "a Python sequence) so that the sync is the caller's choice")
        if counts.dim() != 1 or counts.dtype.is_floating_point or \
                counts.dtype == torch.bool:
            raise ValueError("ft_grouped_linear: counts must be a 1-D integer "
                             "tensor")
        counts = counts.tolist()
    try:
        counts = [operator.index(c) for c in counts]
    except TypeError:
        raise ValueError("ft_grouped_linear: counts must hold integers")
    if len(counts) != experts:
        raise ValueError(f"ft_grouped_linear: {len(counts)} counts for "
                         f"{experts} experts")
    if any(c < 0 for c in counts):
        raise ValueError("ft_grouped_linear: a count is negative")
    if sum(counts) != tokens:
        raise ValueError(f"ft_grouped_linear: counts sum to {sum(counts)}, x "
                         f"has {tokens} rows")
    return counts


def _check(x, weight, counts, bias):
    """Shape, dtype and count rules of ft_grouped_linear; touches no
    extension.  Returns counts as a list of ints."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"ft_grouped_linear: {name} must be float32, "
                             f"got {t.dtype}")
    if weight.dim() != 3:
        raise ValueError(f"ft_grouped_linear: weight must be (E, out, in), "
                         f"got {tuple(weight.shape)}")
    experts, out, inner = weight.shape
    if x.dim() != 2 or x.shape[1] != inner:
        raise ValueError(f"ft_grouped_linear: x must be (T, {inner}), got "
                         f"{tuple(x.shape)}")
    if bias is not None and tuple(bias.shape) != (experts, out):
        raise ValueError(f"ft_grouped_linear: bias must be ({experts}, "
                         f"{out}), got {tuple(bias.shape)}")
    counts = _counts(counts, experts, x.shape[0])
    if x.numel() == 0 or weight.numel() == 0:
        raise ValueError("ft_grouped_linear: empty x or weight")
    return counts


def _split(t: torch.Tensor, counts):
    """The experts' runs of rows of the 2-D t, as views."""
    out, row = [], 0
    for n in counts:
        out.append(t[row:row + n])
        row += n
    return out


def _product(a_list, b_list, c_list, beta, trans_a, trans_b, inject, report,
             tier, streamk):
    from . import (choose_tier_grouped, ft_sgemm_grouped, grouped_layout,
                   grouped_streamk_gate)
    from .ragged_streamk import has_streamk
    shapes = grouped_layout(a_list, b_list, c_list, trans_a, trans_b)
    if tier is None:
        tier = choose_tier_grouped(shapes)
    # stream-K at the device grid: "always" wherever the tier has a twin and
    # the group has units, True where the gate says so
    has_units = any(s[0] > 0 and s[1] > 0 for s in shapes)
    sk = has_streamk(tier) and has_units and (
        streamk == "always" or
        (streamk is True and grouped_streamk_gate(tier, shapes, True)))
    ft_sgemm_grouped(tier, a_list, b_list, c_list, 1.0, beta, inject=inject,
                     report=report, trans_a=trans_a, trans_b=trans_b,
                     streamk="auto" if sk else 0)


class _FTGroupedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, counts, inject, report, tier, streamk):
        x2 = _rows(x)
        w = weight if weight.stride(2) == 1 and \
            weight.stride(1) >= weight.shape[2] else weight.contiguous()
        tokens, out = x2.shape[0], w.shape[1]
        ids = None
        if bias is not None:
            # the expert of every row, built on the host from counts
            ids = torch.repeat_interleave(
                torch.arange(len(counts)),
                torch.tensor(counts)).to(x.device, non_blocking=True)
            y = bias.detach()[ids]
        else:
            y = torch.empty((tokens, out), dtype=x.dtype, device=x.device)
        _product(list(w.unbind(0)), _split(x2, counts), _split(y, counts),
                 0.0 if bias is None else 1.0, True, True, inject, report,
                 tier, streamk)
        ctx.save_for_backward(x2, w, ids)
        ctx.cfg = (counts, inject, report, tier, streamk)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x2, w, ids = ctx.saved_tensors
        counts, inject, report, tier, streamk = ctx.cfg
        g = _rows(grad_y)
        g_list = _split(g, counts)
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.empty_like(x2,
                                      memory_format=torch.contiguous_format)
            _product(list(w.unbind(0)), g_list, _split(grad_x, counts), 0.0,
                     False, True, inject, report, tier, streamk)
        if ctx.needs_input_grad[1]:
            grad_w = torch.empty_like(w, memory_format=torch.contiguous_format)
            _product(_split(x2, counts), g_list, list(grad_w.unbind(0)), 0.0,
                     False, False, inject, report, tier, streamk)
        if ids is not None and ctx.needs_input_grad[2]:
            grad_b = torch.zeros((len(counts), g.shape[1]), dtype=g.dtype,
                                 device=g.device).index_add_(0, ids, g)
        return grad_x, grad_w, grad_b, None, None, None, None, None


def ft_grouped_linear(x: torch.Tensor, weight: torch.Tensor, counts,
                      bias: torch.Tensor | None = None, *,
                      inject: bool = False,
                      report: BatchedFaultReport | None = None,
                      tier: str | None = None,
                      streamk=False) -> torch.Tensor:
    """y[rows of expert e] = x[rows of e] @ weight[e]^T + bias[e] on the
    grouped fused-ABFT SGEMM, differentiable.

    x (T, in) with its rows sorted by expert, weight (E, out, in), bias
    (E, out) or None: fp32 CUDA tensors; y is (T, out).  counts: a Python
    sequence or a CPU integer tensor of E non-negative token counts that sum
    to T; expert e owns the counts[e] rows after those of the experts before
    it.  A CUDA counts tensor is refused: the per-expert shapes are needed on
    the host, and the synchronising copy is left to the caller.

    The forward product and the two backward products (grad_x, grad_weight)
    are one ft_sgemm_grouped launch pair each, whatever E is, and read x,
    weight and the incoming gradient where they lie; only the gradients
    autograd asks for are computed.  With a bias, y is pre-filled with each
    row's bias and the product runs with beta = 1.  An expert with no tokens
    costs no tiles in y and grad_x and gets an exactly zero grad_weight.
    grad_bias is a plain torch segment sum (index_add_), not ABFT-covered.

    inject: run the kernels' injector self-test in every product.
    report: one BatchedFaultReport of E entries that accumulates over all
    products; expert e reports into slot e.
    tier: a tier name for every product; None picks choose_tier_grouped per
    product.
    streamk: False (the default) runs every product as the classic grouped
    launch.  True lets each of the three products take the grouped stream-K
    launch at the device grid where ops.grouped_streamk_gate says it is
    expected to win (GROUPED_STREAMK_NOTE; the candidate is grad_weight,
    whose K is the experts' token counts).  "always" takes it on every
    product whose tier has a stream-K twin (large, huge), whatever the gate
    says.  Split tiles then differ from the classic launch in summation
    order only."""
    if streamk not in (False, True, "always"):
        raise ValueError(f"ft_grouped_linear: streamk must be False, True or "
                         f"'always', got {streamk!r}")
    counts = _check(x, weight, counts, bias)
    return _FTGroupedLinearFn.apply(x, weight, bias, counts, inject, report,
                                    tier, streamk)
