"""The scalar contract C = alpha * A B^T + beta * C0, the parts that need
no GPU: the derived error bound of ft_sgemm_amd/utils/errbound.py (three
independent fp32 products must stay inside it, two deliberately wrong
results must not — the bound is neither too tight nor vacuous), and
beta == 0 not reading C on the CPU panel GEMM of the distributed path.
"""

import numpy as np
import pytest
import torch

from ft_sgemm_amd import ops
from ft_sgemm_amd.ops import golden
from ft_sgemm_amd.parallel.distributed import block_row_sgemm, torch_gemm_fn
from ft_sgemm_amd.utils import errbound as eb

SHAPES = [(64, 48, 192), (64, 48, 640)]
PAIRS = [(0.5, 0.0), (-2.0, 1.0), (0.5, -1.5)]


def _case(m, n, k):
    a, b, _ = ops.make_operands(m, n, k, device="cpu")
    g = torch.Generator(device="cpu").manual_seed(1234)
    c0 = torch.randn((n, m), generator=g)
    return a, b, c0


@pytest.mark.parametrize("alpha,beta", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_products_stay_inside_bound(shape, alpha, beta):
    m, n, k = shape
    a, b, c0 = _case(m, n, k)
    ref = eb.ref64(a, b, c0, alpha, beta)
    e = eb.bound(a, b, c0, alpha, beta, k)
    assert ref.dtype == torch.float64 and e.dtype == torch.float64
    assert ref.shape == e.shape == (n, m) and bool((e > 0).all())

    an, bn, cn = a.numpy(), b.numpy(), c0.numpy()
    gold = golden.sgemm_golden(an.T, bn.T, cn.T, alpha, beta).T
    npy = (np.float32(alpha) * (bn.T @ an) + np.float32(beta) * cn)
    assert gold.dtype == npy.dtype == np.float32
    tch = ops.torch_reference(a, b, c0, alpha, beta)
    for name, got in [("golden", torch.from_numpy(np.ascontiguousarray(gold))),
                      ("numpy", torch.from_numpy(npy)), ("torch", tch)]:
        eb.assert_within(got, ref, e, f"{name} {shape} {alpha} {beta}")


@pytest.mark.parametrize("alpha,beta", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bound_rejects_wrong_results(shape, alpha, beta):
    """One dropped k-term, and alpha applied twice, fall outside E."""
    m, n, k = shape
    a, b, c0 = _case(m, n, k)
    ref = eb.ref64(a, b, c0, alpha, beta)
    e = eb.bound(a, b, c0, alpha, beta, k)
    kd = k // 3
    dropped = ref - alpha * torch.outer(b[kd].double(), a[kd].double())
    doubled = eb.ref64(a, b, c0, 2 * alpha, beta)
    for name, got in [("dropped k-term", dropped), ("doubled alpha", doubled)]:
        outside = (got - ref).abs() > e
        assert outside.double().mean().item() > 0.8, name
        with pytest.raises(AssertionError, match="worst diff/E"):
            eb.assert_within(got, ref, e, name)


def test_ref_and_bound_ignore_c0_at_beta_zero():
    a, b, c0 = _case(64, 48, 192)
    bad = torch.full_like(c0, float("nan"))
    assert torch.equal(eb.ref64(a, b, bad, 0.5, 0.0),
                       eb.ref64(a, b, c0, 0.5, 0.0))
    assert torch.equal(eb.ref64(a, b, None, 0.5, 0.0),
                       eb.ref64(a, b, c0, 0.5, 0.0))
    assert torch.equal(eb.bound(a, b, bad, 0.5, 0.0, 192),
                       eb.bound(a, b, c0, 0.5, 0.0, 192))
    assert torch.isfinite(eb.bound(a, b, bad, 0.5, 0.0, 192)).all()


def test_non_finite_result_is_outside_any_bound():
    a, b, c0 = _case(64, 48, 192)
    ref = eb.ref64(a, b, c0, 1.0, 0.0)
    e = eb.bound(a, b, c0, 1.0, 0.0, 192)
    got = ref.float()
    got[7, 5] = float("nan")
    w, idx = eb.worst_ratio(got, ref, e)
    assert w == float("inf") and idx == (7, 5)
    got[7, 5] = float("inf")
    assert eb.worst_ratio(got, ref, e) == (float("inf"), (7, 5))


@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_torch_gemm_fn_beta_zero_never_reads_c(fill):
    m, n, k = 64, 48, 192
    a, b, c0 = _case(m, n, k)
    ref = eb.ref64(a, b, None, 0.5, 0.0)
    e = eb.bound(a, b, None, 0.5, 0.0, k)
    c = torch.full((n, m), fill)
    torch_gemm_fn(a, b, c, 0.5, 0.0)
    eb.assert_within(c, ref, e, f"torch_gemm_fn fill={fill}")
    # through the panel loop: beta on panel 0 only, alpha on every panel
    c = torch.full((n, m), fill)
    block_row_sgemm(a, b, c, panel_k=64, gemm_fn=torch_gemm_fn, alpha=0.5,
                    beta=0.0)
    eb.assert_within(c, ref, e, f"block_row_sgemm fill={fill}")


def test_torch_gemm_fn_beta_nonzero_unchanged():
    m, n, k = 64, 48, 192
    a, b, c0 = _case(m, n, k)
    c = c0.clone()
    torch_gemm_fn(a, b, c, -2.0, -1.5)
    eb.assert_within(c, eb.ref64(a, b, c0, -2.0, -1.5),
                     eb.bound(a, b, c0, -2.0, -1.5, k), "torch_gemm_fn")
