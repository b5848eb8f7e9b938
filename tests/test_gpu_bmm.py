"""GPU tests of ops.ft_bmm: out = x @ y over a batch with the forward product
and both backward products on the strided-batched ragged fused-ABFT SGEMM,
no operand copied.

Reference: torch.bmm / torch.matmul and their autograd in fp64.  As in
tests/test_gpu_linear.py each product is held to the derived bound of
utils/errbound.py for its own K, (K + 8) * 2^-23 * |x| @ |y|; a corrected
injected fault adds the project's 1e-2 per predicted site (alpha = 1 here).
The gradient of a 2-D shared operand is a plain fp32 sum of B such products:
B more roundings on the summed magnitudes.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.ops.fault_report import predict_injected_events
from ft_sgemm_amd.utils import errbound as eb

B, P, Q, R = 3, 37, 80, 129
FAULT_TOL = 1e-2
# (m, n, k) of out, grad_x and grad_y in the kernels' convention
PRODUCTS = ((R, P, Q), (Q, P, R), (R, Q, P))


def rand(g, *shape):
    return (torch.rand(shape, generator=g) * 1.8 - 0.9).cuda()


_data = {}


def data():
    """(x, y, g) fp32 on the GPU, made once and never written."""
    if not _data:
        g = torch.Generator(device="cpu").manual_seed(4321)
        _data["v"] = (rand(g, B, P, Q), rand(g, B, Q, R), rand(g, B, P, R))
    return _data["v"]


def reference(x, y, g):
    """fp64 (out, grad_x, grad_y) of torch.matmul and its autograd."""
    xd = x.double().requires_grad_()
    yd = y.double().requires_grad_()
    out = torch.matmul(xd, yd)
    out.backward(g.double())
    return out.detach(), xd.grad, yd.grad


def prod_bound(u, v, k, terms=0):
    """(k + 8 + terms) * EPS * |u| @ |v|: errbound.bound with alpha = 1,
    beta = 0, over a batch."""
    return (k + 8 + terms) * eb.EPS * torch.matmul(u.double().abs(),
                                                   v.double().abs())


def bounds(x, y, g):
    t = lambda u: u.transpose(-1, -2)  # noqa: E731
    return (prod_bound(x, y, Q), prod_bound(g, t(y), R),
            prod_bound(t(x), g, P))


def tier_of(tier, m, n, k):
    return tier or ops.choose_tier_ragged_batched(m, n, k, B)


def sites(tier):
    """Predicted in-range injected sites of the three products (the same in
    every entry), as fp64 count tensors shaped like one entry of out, grad_x
    and grad_y."""
    out = []
    for m, n, k in PRODUCTS:
        v = torch.zeros((n, m), dtype=torch.float64)
        for e in predict_injected_events(tier_of(tier, m, n, k), m, n, k,
                                         ragged=True):
            if e.i < m and e.j < n:
                v[e.j, e.i] += 1
        out.append(v.cuda())
    return out


def run(x, y, g, **kw):
    xr = x.clone().requires_grad_()
    yr = y.clone().requires_grad_()
    out = ops.ft_bmm(xr, yr, **kw)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), xr.grad, yr.grad


@pytest.mark.parametrize("tier", [None, "huge"])
def test_matches_torch_bmm(tier):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    x, y, g = data()
    out, gx, gy = run(x, y, g, tier=tier)
    assert out.shape == (B, P, R)
    r_out, r_gx, r_gy = reference(x, y, g)
    e_out, e_gx, e_gy = bounds(x, y, g)
    eb.assert_within(out, r_out, e_out, f"out tier={tier}")
    eb.assert_within(gx, r_gx, e_gx, f"grad_x tier={tier}")
    eb.assert_within(gy, r_gy, e_gy, f"grad_y tier={tier}")


@pytest.mark.parametrize("tier", [None, "huge"])
def test_injected_faults_are_corrected(tier):
    x, y, g = data()
    rep = ops.BatchedFaultReport(B)
    out, gx, gy = run(x, y, g, tier=tier, inject=True, report=rep)
    want = sum(len(predict_injected_events(tier_of(tier, m, n, k), m, n, k,
                                           ragged=True))
               for m, n, k in PRODUCTS)
    assert want > 0
    for r in rep.read():
        assert r.n_events == r.corrected == want
        assert r.uncorrected == r.unlocated == r.dropped == 0
    r_out, r_gx, r_gy = reference(x, y, g)
    e_out, e_gx, e_gy = bounds(x, y, g)
    s_out, s_gx, s_gy = sites(tier)
    eb.assert_within(out, r_out, e_out + FAULT_TOL * s_out, "out inject")
    eb.assert_within(gx, r_gx, e_gx + FAULT_TOL * s_gx, "grad_x inject")
    eb.assert_within(gy, r_gy, e_gy + FAULT_TOL * s_gy, "grad_y inject")


@pytest.fixture
def launches(monkeypatch):
    """Every ft_sgemm_ragged_batched call ft_bmm makes, as (a, b) data
    pointers, by wrapping the function ft_bmm looks up."""
    seen = []
    real = ops.ft_sgemm_ragged_batched

    def wrapper(tier, a, b, c, *args, **kw):
        seen.append((a.data_ptr(), b.data_ptr()))
        return real(tier, a, b, c, *args, **kw)

    monkeypatch.setattr(ops, "ft_sgemm_ragged_batched", wrapper)
    return seen


def test_views_are_read_in_place(launches):
    """Attention scores on head views: q heads (H, T, D) of a (T, H, D)
    tensor and keys as a transpose(1, 2) view.  Forward and backward read the
    tensors where they lie and give the bits of the contiguous copies."""
    heads, t_, d = 3, 41, 80
    gen = torch.Generator(device="cpu").manual_seed(77)
    q_thd = rand(gen, t_, heads, d).requires_grad_()
    k_thd = rand(gen, t_, heads, d).requires_grad_()
    g = rand(gen, heads, t_, t_)
    q = q_thd.permute(1, 0, 2)                  # (H, T, D), row stride H*D
    kt = k_thd.permute(1, 0, 2).transpose(1, 2)  # (H, D, T), unit stride on D
    assert not q.is_contiguous() and kt.stride(1) == 1
    out = ops.ft_bmm(q, kt)
    out.backward(g)
    torch.cuda.synchronize()
    qp, kp = q_thd.data_ptr(), k_thd.data_ptr()
    assert len(launches) == 3
    assert launches[0] == (kp, qp)  # out: a = y, b = x
    assert launches[1][0] == kp     # grad_x: a = y
    assert launches[2][1] == qp     # grad_y: b = x
    qc = q.detach().contiguous().requires_grad_()
    kc = kt.detach().contiguous().requires_grad_()
    want = ops.ft_bmm(qc, kc)
    want.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want.detach())
    assert torch.equal(q_thd.grad.permute(1, 0, 2), qc.grad)
    assert torch.equal(k_thd.grad.permute(1, 2, 0), kc.grad)
    qd, kd = q.detach(), kt.detach()
    eb.assert_within(out.detach(), torch.matmul(qd.double(), kd.double()),
                     prod_bound(qd, kd, d), "scores")


def test_shared_2d_y():
    """A 2-D y is shared by the batch; its gradient is summed over it."""
    x, y, g = data()
    out, gx, gy = run(x, y[1], g)
    assert gy.shape == (Q, R)
    r_out, r_gx, r_gy = reference(x, y[1], g)
    assert r_gy.shape == (Q, R)
    eb.assert_within(out, r_out, prod_bound(x, y[1], Q), "shared y out")
    eb.assert_within(gx, r_gx, prod_bound(g, y[1].t(), R), "shared y grad_x")
    e_gy = prod_bound(x.transpose(1, 2), g, P, terms=B).sum(dim=0)
    eb.assert_within(gy, r_gy, e_gy, "shared y grad_y")


def test_only_requested_gradients_are_computed(launches):
    x, y, g = data()
    ops.ft_bmm(x, y)
    assert len(launches) == 1
    for x_grad, y_grad, n in ((True, False, 2), (False, True, 2),
                              (True, True, 3)):
        del launches[:]
        xr = x.clone().requires_grad_(x_grad)
        yr = y.clone().requires_grad_(y_grad)
        ops.ft_bmm(xr, yr).backward(g)
        assert len(launches) == n
        assert (xr.grad is not None) == x_grad
        assert (yr.grad is not None) == y_grad
    torch.cuda.synchronize()
