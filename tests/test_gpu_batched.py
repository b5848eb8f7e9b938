"""GPU tests of the strided-batched plain and fused-ABFT SGEMM.

One shape rule for every test: M = 2*bm, N = 3*bn, K = 128, batch = 3 —
more than one block in x, y and z with unequal x and y counts (swapped
indices show), two 64-k strip windows and at least 4 panels on every tier,
and with K / bkf < 20 panels every panel is a verify window.  alpha = 1.25,
beta = -1.5, C prefilled with seeded random values, every entry different.

The per-entry references are today's single launches with stream-K off
(FT_SGEMM_STREAMK=0): a batched launch always takes the classic
decomposition, and the fused huge tier would otherwise auto-engage stream-K
at these tile counts and sum in another order.  Against them the batched
result must be BIT-identical: same kernel body, same tiles, same order.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING

ABS_TOL = 1e-2  # tests/test_gpu_kernels.py
REL_TOL = 1e-2
BATCH, K = 3, 128
ALPHA, BETA = 1.25, -1.5
GAP = 8  # floats between entries of the padded layouts

MODES = {
    "plain": None,
    "fused": dict(inject=False),
    "fused_inject": dict(inject=True),
}


def shape(tier):
    t = TILING[tier]
    return 2 * t["bm"], 3 * t["bn"], K


def check(ref, got):
    diff = (ref - got).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


def run_single(tier, mode, a, b, c, **kw):
    if MODES[mode] is None:
        return ops.sgemm(tier, a, b, c, ALPHA, BETA)
    return ops.ft_sgemm(tier, a, b, c, ALPHA, BETA, **MODES[mode], **kw)


def run_batched(tier, mode, a, b, c, **kw):
    if MODES[mode] is None:
        return ops.sgemm_batched(tier, a, b, c, ALPHA, BETA)
    return ops.ft_sgemm_batched(tier, a, b, c, ALPHA, BETA, **MODES[mode],
                                **kw)


_operands = {}


def operands(tier):
    """Seeded (a, b, c0) of the common shape, made once per tier and never
    written to."""
    if tier not in _operands:
        m, n, k = shape(tier)
        g = torch.Generator(device="cpu").manual_seed(1234 + TIERS.index(tier))
        a = (torch.rand((BATCH, k, m), generator=g) * 1.8 - 0.9).cuda()
        b = (torch.rand((BATCH, k, n), generator=g) * 1.8 - 0.9).cuda()
        c0 = torch.randn((BATCH, n, m), generator=g).cuda()
        _operands[tier] = (a, b, c0)
    return _operands[tier]


_singles = {}


def singles(tier, mode, monkeypatch, a=None, b=None):
    """Per-entry single-launch results (classic path), stacked (B, N, M);
    cached for the shared operands."""
    monkeypatch.setenv("FT_SGEMM_STREAMK", "0")
    shared = a is None and b is None
    if shared and (tier, mode) in _singles:
        return _singles[(tier, mode)]
    a0, b0, c0 = operands(tier)
    a = a0 if a is None else a
    b = b0 if b is None else b
    out = c0.clone()
    for i in range(BATCH):
        run_single(tier, mode, a[i].contiguous(), b[i].contiguous(), out[i])
    torch.cuda.synchronize()
    if shared:
        _singles[(tier, mode)] = out
    return out


def padded(x, fill):
    """x (B, R, C) copied into a flat buffer with GAP floats after every
    entry, the gaps holding `fill`.  Returns (view, flat, gap mask)."""
    bsz, r, c = x.shape
    step = r * c + GAP
    flat = torch.full((bsz * step,), fill, device=x.device)
    view = flat.as_strided((bsz, r, c), (step, c, 1))
    view.copy_(x)
    mask = torch.ones(bsz * step, dtype=torch.bool, device=x.device)
    mask.as_strided((bsz, r, c), (step, c, 1)).fill_(False)
    return view, flat, mask


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tier", TIERS)
def test_bit_identical_to_single_launches(tier, mode, monkeypatch):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    a, b, c0 = operands(tier)
    want = singles(tier, mode, monkeypatch)
    c = c0.clone()
    run_batched(tier, mode, a, b, c)
    torch.cuda.synchronize()
    for i in range(BATCH):
        assert torch.equal(c[i], want[i]), (
            f"entry {i}: {int((c[i] != want[i]).sum())} elements differ from "
            f"the single launch")
    check(ops.torch_reference_batched(a, b, c0, ALPHA, BETA), c)


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_padded_strides(tier, mode, monkeypatch):
    a, b, c0 = operands(tier)
    want = singles(tier, mode, monkeypatch)
    sentinel = -12345.0
    ap, _, _ = padded(a, float("nan"))
    bp, _, _ = padded(b, float("nan"))
    cp, cflat, cgap = padded(c0, sentinel)
    assert ops.batched_layout(ap, bp, cp)[4:] == tuple(
        x[0].numel() + GAP for x in (a, b, c0))
    run_batched(tier, mode, ap, bp, cp)
    torch.cuda.synchronize()
    assert torch.equal(cp, want)
    assert int(cgap.sum()) == BATCH * GAP
    assert bool((cflat[cgap] == sentinel).all()), "a gap of C was written"


@pytest.mark.parametrize("tier", TIERS)
def test_broadcast_operands(tier, monkeypatch):
    """expand()ed (stride 0) and 2-D operands, fused with injection, equal
    the run on materialised copies; a shared A asks for one matrix's
    workspace."""
    a, b, c0 = operands(tier)
    m, n, k = shape(tier)
    ext = ops._require_ext()
    ti = ops.tier_index(tier)

    a_sh = a[1].expand(BATCH, k, m)
    assert a_sh.stride(0) == 0
    a_mat = a_sh.contiguous()
    want = singles(tier, "fused_inject", monkeypatch, a=a_mat)
    c_mat = c0.clone()
    run_batched(tier, "fused_inject", a_mat, b, c_mat)
    for a_in in (a_sh, a[1]):
        c = c0.clone()
        run_batched(tier, "fused_inject", a_in, b, c)
        torch.cuda.synchronize()
        assert torch.equal(c, c_mat) and torch.equal(c, want)
    one = ext.batched_workspace_floats(ti, a[:1], b[:1], c0[:1])
    assert one > 0
    assert ext.batched_workspace_floats(ti, a_sh, b, c0) == one
    assert ext.batched_workspace_floats(ti, a_mat, b, c0) == BATCH * one

    b_sh = b[2].expand(BATCH, k, n)
    b_mat = b_sh.contiguous()
    want = singles(tier, "fused_inject", monkeypatch, b=b_mat)
    for b_in in (b_sh, b[2], b_mat):
        c = c0.clone()
        run_batched(tier, "fused_inject", a, b_in, c)
        torch.cuda.synchronize()
        assert torch.equal(c, want)


@pytest.mark.parametrize("tier", ["huge", "tall", "small"])
def test_report_per_entry(tier, monkeypatch):
    """Every entry logs its own injections into its own slot."""
    a, b, c0 = operands(tier)
    m, n, k = shape(tier)
    want = singles(tier, "fused_inject", monkeypatch)
    expect = ops.predict_injected_events(tier, m, n, k)
    rep = ops.BatchedFaultReport(BATCH)
    c = c0.clone()
    run_batched(tier, "fused_inject", a, b, c, report=rep)
    got = rep.read()
    c_plain_log = c0.clone()
    run_batched(tier, "fused_inject", a, b, c_plain_log)
    assert torch.equal(c, c_plain_log), "C changed with a report attached"
    assert torch.equal(c, want)
    assert len(got) == BATCH
    for i, r in enumerate(got):
        assert r.n_events == len(expect) and r.corrected == len(expect), i
        assert r.uncorrected == 0 and r.unlocated == 0 and r.dropped == 0, i
        assert len(r.events) == len(expect)
        for e, w in zip(r.events, expect):
            assert e[:5] == w[:5] and e[6:] == w[6:], (i, e, w)
            # rc - inj_mag is the error left in C, held to ABS_TOL
            assert abs(e.magnitude - w.magnitude) <= ABS_TOL
    rep.raise_if_uncorrected()
    rep.reset()
    assert all(r.n_events == 0 for r in rep.read())


@pytest.mark.parametrize("tier", ["huge", "medium"])
def test_batch_of_one_is_the_single_launch(tier):
    """batch == 1 takes today's path (stream-K gates included)."""
    a, b, c0 = operands(tier)
    for mode in MODES:
        c_s = c0[0].clone()
        run_single(tier, mode, a[0], b[0], c_s)
        c_b = c0[:1].clone()
        run_batched(tier, mode, a[:1], b[:1], c_b)
        torch.cuda.synchronize()
        assert torch.equal(c_b[0], c_s), mode


def test_binding_rejects_bad_launches():
    tier = "medium"
    ext = ops._require_ext()
    ti = ops.tier_index(tier)
    a, b, c0 = operands(tier)
    m, n, k = shape(tier)
    args = (1.0, 0.0, 0.0, 0.0, 20)
    # batch stride of a not a multiple of 4 floats
    step = k * m + 2
    a_bad = torch.zeros(BATCH * step, device="cuda").as_strided(
        (BATCH, k, m), (step, m, 1))
    c = c0.clone()
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ext.sgemm_batched(ti, False, False, a_bad, b, c, *args)
    # M not a multiple of the tile
    a16 = a[:, :, :16].contiguous()
    c16 = c0[:, :, :16].contiguous()
    c16_0 = c16.clone()
    with pytest.raises(RuntimeError, match="multiples of its tile"):
        ext.sgemm_batched(ti, False, False, a16, b, c16, *args)
    torch.cuda.synchronize()
    assert torch.equal(c, c0) and torch.equal(c16, c16_0)
