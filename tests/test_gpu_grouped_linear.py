"""GPU tests of ops.ft_grouped_linear: E expert layers over the expert-sorted
rows of x, forward and both backward products one grouped fused-ABFT launch
each.

Reference: a per-expert loop of torch.nn.functional.linear and its autograd in
fp64.  As in tests/test_gpu_linear.py each product is held to the derived
bound of utils/errbound.py for its own K (in, out, and the expert's token
count), and grad_bias, a plain fp32 sum of the expert's tokens in any order,
to (tokens + 8) * EPS * sum |grad_y|.  The second reference is a per-expert
loop of ops.ft_linear on the same tier, which runs the same kernels per entry:
bit for bit.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.utils import errbound as eb

E, COUNTS, IN, OUT = 4, [5, 0, 33, 1], 40, 24
T = sum(COUNTS)
STARTS = [sum(COUNTS[:e]) for e in range(E)]

_data = {}


def data():
    """(x, w, bias, gy) fp32 on the GPU, made once and never written."""
    if not _data:
        g = torch.Generator(device="cpu").manual_seed(2468)
        r = lambda *s: (torch.rand(s, generator=g) * 1.8 - 0.9).cuda()  # noqa
        _data["v"] = (r(T, IN), r(E, OUT, IN), r(E, OUT), r(T, OUT))
    return _data["v"]


def rows(t, e):
    return t[STARTS[e]:STARTS[e] + COUNTS[e]]


def run(x, w, bias, gy, **kw):
    xr = x.clone().requires_grad_()
    wr = w.clone().requires_grad_()
    br = None if bias is None else bias.clone().requires_grad_()
    y = ops.ft_grouped_linear(xr, wr, COUNTS, br, **kw)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xr.grad, wr.grad, None if br is None else br.grad


def expert_loop(fn, x, w, bias, gy, dtype):
    """(y, gx, gw, gb) of fn = F.linear-like applied expert by expert, with
    autograd, in dtype.  An expert without tokens gets zero gradients."""
    leaf = lambda t: t.to(dtype).clone().requires_grad_()  # noqa: E731
    xd, wd = leaf(x), leaf(w)
    bd = None if bias is None else leaf(bias)
    parts = []
    for e in range(E):
        if COUNTS[e]:
            parts.append(fn(rows(xd, e), wd[e], None if bd is None else bd[e]))
    y = torch.cat(parts)
    y.backward(gy.to(dtype))
    torch.cuda.synchronize()
    return (y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad)


@pytest.mark.parametrize("with_bias", [False, True])
def test_matches_functional_linear(with_bias):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    x, w, bias, gy = data()
    bias = bias if with_bias else None
    y, gx, gw, gb = run(x, w, bias, gy)
    assert y.shape == (T, OUT) and gw.shape == (E, OUT, IN)
    ry, rgx, rgw, rgb = expert_loop(F.linear, x, w, bias, gy, torch.float64)
    for e in range(E):
        n = COUNTS[e]
        if n == 0:
            continue
        xe, ge = rows(x, e), rows(gy, e)
        c0 = None if bias is None else bias[e].expand(n, -1)
        # the three products in the kernel's (K, M) / (K, N) / (N, M) terms
        ey = eb.bound(w[e].t(), xe.t(), c0, 1.0, 0.0 if bias is None else 1.0,
                      IN)
        egx = eb.bound(w[e], ge.t(), None, 1.0, 0.0, OUT)
        egw = eb.bound(xe, ge, None, 1.0, 0.0, n)
        eb.assert_within(rows(y, e), rows(ry, e), ey, f"y expert {e}")
        eb.assert_within(rows(gx, e), rows(rgx, e), egx, f"grad_x expert {e}")
        eb.assert_within(gw[e], rgw[e], egw, f"grad_w expert {e}")
        if with_bias:
            eg = (n + 8) * eb.EPS * ge.double().abs().sum(dim=0)
            eb.assert_within(gb[e], rgb[e], eg, f"grad_bias expert {e}")
    if not with_bias:
        assert gb is None


@pytest.mark.parametrize("tier", ["medium", "huge"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_bits_of_a_per_expert_ft_linear_loop(with_bias, tier):
    x, w, bias, gy = data()
    bias = bias if with_bias else None
    y, gx, gw, gb = run(x, w, bias, gy, tier=tier)
    fn = lambda xe, we, be: ops.ft_linear(xe, we, be, tier=tier)  # noqa: E731
    ly, lgx, lgw, lgb = expert_loop(fn, x, w, bias, gy, torch.float32)
    assert torch.equal(y, ly)
    assert torch.equal(gx, lgx)
    for e in range(E):
        if COUNTS[e]:
            assert torch.equal(gw[e], lgw[e]), f"grad_w expert {e}"


@pytest.mark.parametrize("with_bias", [False, True])
def test_expert_without_tokens_gets_exact_zero_gradients(with_bias):
    x, w, bias, gy = data()
    _, _, gw, gb = run(x, w, bias if with_bias else None, gy)
    empty = COUNTS.index(0)
    assert torch.equal(gw[empty], torch.zeros_like(gw[empty]))
    assert not torch.equal(gw[0], torch.zeros_like(gw[0]))
    if with_bias:
        assert torch.equal(gb[empty], torch.zeros_like(gb[empty]))


def test_injected_faults_are_corrected():
    x, w, bias, gy = data()
    rep = ops.BatchedFaultReport(E)
    y, gx, gw, _ = run(x, w, bias, gy, inject=True, report=rep)
    got = rep.read()
    assert sum(r.corrected for r in got) > 0
    for e, r in enumerate(got):
        assert r.uncorrected == r.unlocated == 0, f"expert {e}"
        assert r.n_events == r.corrected
    assert got[0].corrected > 0 and got[2].corrected > 0
    # corrected means corrected: the clean run's values within the project's
    # 1e-2 per injected site (alpha = 1)
    cy, cgx, cgw, _ = run(x, w, bias, gy)
    n_sites = max(r.corrected for r in got)
    for a, b in ((y, cy), (gx, cgx), (gw, cgw)):
        assert (a - b).abs().max().item() <= 1e-2 * n_sites


@pytest.fixture
def launches(monkeypatch):
    """Every ft_sgemm_grouped call ft_grouped_linear makes, as
    (entries, trans_a, trans_b), by wrapping the function it looks up."""
    seen = []
    real = ops.ft_sgemm_grouped

    def wrapper(tier, a_list, b_list, c_list, *args, **kw):
        seen.append((len(c_list), kw.get("trans_a"), kw.get("trans_b")))
        return real(tier, a_list, b_list, c_list, *args, **kw)

    monkeypatch.setattr(ops, "ft_sgemm_grouped", wrapper)
    return seen


def test_one_grouped_launch_per_product(launches):
    x, w, bias, gy = data()
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = ops.ft_grouped_linear(xr, wr, torch.tensor(COUNTS), bias)
    assert launches == [(E, True, True)]          # y: TT
    y.backward(gy)
    torch.cuda.synchronize()
    assert launches[1:] == [(E, False, True),     # grad_x: NT
                            (E, False, False)]    # grad_weight: untransposed


def test_cuda_counts_are_refused():
    x, w, _, _ = data()
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.ft_grouped_linear(x, w, torch.tensor(COUNTS).cuda())
