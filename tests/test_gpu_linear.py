"""GPU tests of ops.ft_linear / ops.FTLinear: y = x @ W^T + bias with the
forward product and both backward products on the fused-ABFT ragged SGEMM,
no operand copied.

Reference: torch.nn.functional.linear and its autograd in fp64.  Each of
the three products is held to the derived bound of utils/errbound.py for its
own K (in, out and tokens); a corrected injected fault adds the project's
|alpha| * 1e-2 per predicted site (alpha = 1 here).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.ops.fault_report import FaultReport, predict_injected_events
from ft_sgemm_amd.utils import errbound as eb

TOKENS, IN, OUT = 37, 70, 131
FAULT_TOL = 1e-2


_data = {}


def data():
    """(x, w, bias, gy) fp32 on the GPU, made once and never written."""
    if not _data:
        g = torch.Generator(device="cpu").manual_seed(1234)
        r = lambda *s: (torch.rand(s, generator=g) * 1.8 - 0.9).cuda()  # noqa
        _data["v"] = (r(TOKENS, IN), r(OUT, IN), r(OUT), r(TOKENS, OUT))
    return _data["v"]


def reference(x, w, bias, gy):
    """fp64 (y, gx, gw, gb) of F.linear and its autograd."""
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    bd = None if bias is None else bias.double().requires_grad_()
    y = F.linear(xd, wd, bd)
    y.backward(gy.double())
    return (y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad)


def bounds(x, w, bias, gy):
    """errbound.bound of each product in the kernel's (K, M) / (K, N) / (N, M)
    convention: y = w x^T over K = in (plus the pre-filled bias, beta = 1),
    gx = gy w over K = out, gw = gy^T x over K = tokens."""
    x2, g2 = x.reshape(-1, x.shape[-1]), gy.reshape(-1, gy.shape[-1])
    tokens = x2.shape[0]
    c0 = None if bias is None else bias.expand(tokens, -1)
    return (eb.bound(w.t(), x2.t(), c0, 1.0, 0.0 if bias is None else 1.0,
                     x2.shape[1]),
            eb.bound(w, g2.t(), None, 1.0, 0.0, w.shape[0]),
            eb.bound(x2, g2, None, 1.0, 0.0, tokens))


def sites(tier_of, tokens):
    """Predicted in-range injected sites of the three products, as fp64
    count tensors shaped like y, gx and gw."""
    out = []
    for m, n, k in ((OUT, tokens, IN), (IN, tokens, OUT), (IN, OUT, tokens)):
        v = torch.zeros((n, m), dtype=torch.float64)
        for e in predict_injected_events(tier_of(m, n, k), m, n, k,
                                         ragged=True):
            if e.i < m and e.j < n:
                v[e.j, e.i] += 1
        out.append(v.cuda())
    return out


def tier_fn(tier):
    return lambda m, n, k: tier or ops.choose_tier(m, n, k, ragged=True)


def run(x, w, bias, gy, **kw):
    xr = x.clone().requires_grad_()
    wr = w.clone().requires_grad_()
    br = None if bias is None else bias.clone().requires_grad_()
    y = ops.ft_linear(xr, wr, br, **kw)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xr.grad, wr.grad, None if br is None else br.grad


@pytest.mark.parametrize("tier", [None, "huge"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_matches_functional_linear(with_bias, tier):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    x, w, bias, gy = data()
    bias = bias if with_bias else None
    y, gx, gw, gb = run(x, w, bias, gy, tier=tier)
    ry, rgx, rgw, rgb = reference(x, w, bias, gy)
    ey, egx, egw = bounds(x, w, bias, gy)
    eb.assert_within(y, ry, ey, f"y tier={tier}")
    eb.assert_within(gx, rgx, egx, f"grad_x tier={tier}")
    eb.assert_within(gw, rgw, egw, f"grad_w tier={tier}")
    if with_bias:
        # a plain fp32 sum of TOKENS terms, any order
        eg = (TOKENS + 8) * eb.EPS * gy.double().abs().sum(dim=0)
        eb.assert_within(gb, rgb, eg, "grad_bias")
    else:
        assert gb is None


@pytest.mark.parametrize("tier", [None, "huge"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_injected_faults_are_corrected(with_bias, tier):
    x, w, bias, gy = data()
    bias = bias if with_bias else None
    rep = FaultReport()
    y, gx, gw, _ = run(x, w, bias, gy, tier=tier, inject=True, report=rep)
    r = rep.read()
    want = sum(len(predict_injected_events(tier_fn(tier)(m, n, k), m, n, k,
                                           ragged=True))
               for m, n, k in ((OUT, TOKENS, IN), (IN, TOKENS, OUT),
                               (IN, OUT, TOKENS)))
    assert r.corrected > 0 and r.uncorrected == r.unlocated == 0
    assert r.n_events == r.corrected == want
    ry, rgx, rgw, _ = reference(x, w, bias, gy)
    ey, egx, egw = bounds(x, w, bias, gy)
    sy, sgx, sgw = sites(tier_fn(tier), TOKENS)
    eb.assert_within(y, ry, ey + FAULT_TOL * sy, "y inject")
    eb.assert_within(gx, rgx, egx + FAULT_TOL * sgx, "grad_x inject")
    eb.assert_within(gw, rgw, egw + FAULT_TOL * sgw, "grad_w inject")


def test_strided_3d_input_is_read_in_place():
    """x as a (2, 19, 70) slice of a wider tensor (inner stride 1) gives the
    bits of its contiguous copy, forward and backward."""
    g = torch.Generator(device="cpu").manual_seed(99)
    wide = (torch.rand((2, 19, IN + 9), generator=g) * 1.8 - 0.9).cuda()
    xs = wide[..., 3:3 + IN]
    assert not xs.is_contiguous() and xs.stride(-1) == 1
    _, w, bias, _ = data()
    gy = (torch.rand((2, 19, OUT), generator=g) * 1.8 - 0.9).cuda()
    got = run(xs, w, bias, gy)
    # run() clones: hand the view itself to ft_linear as well
    xv = xs.detach().requires_grad_()
    assert not xv.is_contiguous()
    yv = ops.ft_linear(xv, w, bias)
    yv.backward(gy)
    want = run(xs.contiguous(), w, bias, gy)
    torch.cuda.synchronize()
    assert got[0].shape == (2, 19, OUT) and got[1].shape == (2, 19, IN)
    assert torch.equal(yv.detach(), want[0])
    assert torch.equal(xv.grad, want[1])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    ry = reference(xs.contiguous(), w, bias, gy)[0]
    eb.assert_within(yv.detach().reshape(-1, OUT), ry.reshape(-1, OUT),
                     bounds(xs.contiguous(), w, bias, gy)[0], "3-D y")


def test_module_matches_nn_linear():
    x, w, bias, gy = data()
    ref = torch.nn.Linear(IN, OUT).cuda()
    lin = ops.FTLinear(IN, OUT, device="cuda")
    with torch.no_grad():
        ref.weight.copy_(w), ref.bias.copy_(bias)
    lin.load_state_dict(ref.state_dict())
    xr = x.clone().requires_grad_()
    y = lin(xr)
    y.backward(gy)
    torch.cuda.synchronize()
    ry, rgx, rgw, rgb = reference(x, w, bias, gy)
    ey, egx, egw = bounds(x, w, bias, gy)
    eb.assert_within(y.detach(), ry, ey, "FTLinear y")
    eb.assert_within(xr.grad, rgx, egx, "FTLinear grad_x")
    eb.assert_within(lin.weight.grad, rgw, egw, "FTLinear grad_w")
    assert lin.bias.grad is not None
    # and the fp32 module agrees within twice the bound (both sides err)
    eb.assert_within(y.detach(), ref(x).double().detach(), 2 * ey,
                     "FTLinear vs nn.Linear")


def test_no_grad_x_product_when_x_needs_none():
    """requires_grad=False on x launches no grad_x product: under injection
    the report then holds the events of two products, not three."""
    x, w, bias, gy = data()
    tf = tier_fn(None)
    n_of = lambda m, n, k: len(predict_injected_events(  # noqa: E731
        tf(m, n, k), m, n, k, ragged=True))
    n_y, n_gx, n_gw = (n_of(OUT, TOKENS, IN), n_of(IN, TOKENS, OUT),
                       n_of(IN, OUT, TOKENS))
    assert n_gx > 0
    rep = FaultReport()
    wr = w.clone().requires_grad_()
    y = ops.ft_linear(x, wr, bias, inject=True, report=rep)
    y.backward(gy)
    r = rep.read()
    assert r.n_events == r.corrected == n_y + n_gw
    assert wr.grad is not None
    # and with x asking for its gradient, the third product reports too
    rep = FaultReport()
    xr = x.clone().requires_grad_()
    y = ops.ft_linear(xr, w, bias, inject=True, report=rep)
    y.backward(gy)
    r = rep.read()
    assert r.n_events == r.corrected == n_y + n_gx
    assert xr.grad is not None
