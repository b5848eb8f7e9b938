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

import math

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


# ---- the launch rules, through the raw bindings ---------------------------
# One statement of the rules (gemm_args_error, csrc/dispatch.hip) and one
# fault-log check behind all three entries: every rule that can be broken
# from tensors is broken once through every entry it applies to.  Medium tier
# at one tile; nothing is launched.

REJ_TIER = "medium"
ENTRIES = ("sgemm", "sgemm_batched", "sgemm_ragged")
TILED = ("sgemm", "sgemm_batched")


def _rej_operands(entry, m=None, n=None, k=None):
    """A launchable call of `entry`: one tile, a batch of BATCH for the
    batched entry.  c is a view of c_flat."""
    t = TILING[REJ_TIER]
    m, n, k = m or t["bm"], n or t["bn"], k or t["bk"]
    lead = (BATCH,) if entry == "sgemm_batched" else ()
    g = torch.Generator(device="cpu").manual_seed(99)

    def rand(*shape):
        return torch.rand(shape, generator=g).cuda()

    c_flat = rand(BATCH * n * m)
    return dict(a=rand(*lead, k, m), b=rand(*lead, k, n), c_flat=c_flat,
                c=c_flat[:math.prod(lead) * n * m].view(*lead, n, m),
                abft=False, log=(None, None))


def _log(entry, device="cuda"):
    lead = (BATCH,) if entry == "sgemm_batched" else ()
    return (torch.full(lead + (5,), 7, dtype=torch.int32, device=device),
            torch.full(lead + (4, 8), 7, dtype=torch.int32, device=device))


def _misfit(dim):
    def build(entry):
        t = TILING[REJ_TIER]
        size = dict(m=t["bm"], n=t["bn"], k=t["bk"])
        size[dim] //= 2  # 16, 16 or 8: still multiples of 4
        return _rej_operands(entry, **size)
    return build


def _stride_not_4(entry):
    d = _rej_operands(entry)
    _, k, m = d["a"].shape
    step = k * m + 2
    d["a"] = torch.zeros(BATCH * step, device="cuda").as_strided(
        (BATCH, k, m), (step, m, 1))
    return d


def _c_entries_overlap(entry):
    d = _rej_operands(entry)
    _, n, m = d["c"].shape
    d["c"] = d["c_flat"].as_strided((BATCH, n, m), (n * m - 4, m, 1))
    return d


def _offset_base(entry):
    d = _rej_operands(entry)
    shape = d["a"].shape
    d["a"] = torch.zeros(d["a"].numel() + 1, device="cuda")[1:].view(shape)
    assert d["a"].data_ptr() % 16 == 4
    return d


def _short_row_stride(which):
    def build(entry):
        d = _rej_operands(entry)
        rows, width = d[which].shape
        d[which] = d["c_flat"].as_strided((rows, width), (width - 1, 1))
        return d
    return build


def _bad_log(how):
    def build(entry):
        d = _rej_operands(entry)
        d["abft"] = how != "plain"
        cn, ev = _log(entry)
        if how == "rank":
            cn = cn.reshape(-1) if cn.dim() == 2 else cn.reshape(1, -1)
        elif how == "dtype":
            cn = cn.long()
        elif how == "device":
            ev = ev.cpu()
        elif how == "alone":
            ev = None
        d["log"] = (cn, ev)
        return d
    return build


def _tile_text(dim):
    t = TILING[REJ_TIER]
    size = dict(m=t["bm"], n=t["bn"], k=t["bk"])
    size[dim] //= 2
    return (r"multiples of its tile.*M={m} N={n} K={k}\b".format(**size))


# name: (entries, text of the error, builder)
REJECTIONS = {
    "misfit_m": (TILED, _tile_text("m"), _misfit("m")),
    "misfit_n": (TILED, _tile_text("n"), _misfit("n")),
    "misfit_k": (TILED, _tile_text("k"), _misfit("k")),
    "stride_not_4": (("sgemm_batched",), "multiples of 4", _stride_not_4),
    "c_entries_overlap": (("sgemm_batched",), "overlap", _c_entries_overlap),
    "offset_base": (("sgemm_batched",), "16-byte aligned", _offset_base),
    "short_row_a": (("sgemm_ragged",), "shorter than", _short_row_stride("a")),
    "short_row_b": (("sgemm_ragged",), "shorter than", _short_row_stride("b")),
    "short_row_c": (("sgemm_ragged",), "shorter than", _short_row_stride("c")),
    "log_rank": (ENTRIES, "fault-log counters must", _bad_log("rank")),
    "log_dtype": (ENTRIES, "must be int32", _bad_log("dtype")),
    "log_device": (ENTRIES, "operands' device", _bad_log("device")),
    "log_alone": (ENTRIES, "go together", _bad_log("alone")),
    "log_on_plain": (ENTRIES, "needs a fused-ABFT kernel", _bad_log("plain")),
}


@pytest.mark.parametrize("entry,case", [
    pytest.param(e, name, id=f"{name}-{e}")
    for name, (entries, _, _) in REJECTIONS.items() for e in entries])
def test_binding_rejects_bad_launches(entry, case):
    _, text, build = REJECTIONS[case]
    d = build(entry)
    watched = [d["c_flat"]] + [x for x in d["log"] if x is not None]
    before = [x.clone() for x in watched]
    with pytest.raises(RuntimeError, match=text):
        getattr(ops._require_ext(), entry)(
            ops.tier_index(REJ_TIER), d["abft"], False, d["a"], d["b"],
            d["c"], 1.0, 0.0, 0.0, 0.0, 20, *d["log"])
    torch.cuda.synchronize()
    for x, x0 in zip(watched, before):
        assert torch.equal(x, x0), "a rejected call wrote to its tensors"


@pytest.mark.parametrize("tier", TIERS)
def test_workspace_query_is_the_formula(tier):
    """2 * ceil(M / wm) * round_up(K, 64) floats, times the batch when every
    entry has an A of its own: the one C++ query behind both bindings."""
    t = TILING[tier]
    bm, bn, bk = t["bm"], t["bn"], t["bk"]
    ext = ops._require_ext()
    ti = ops.tier_index(tier)

    def want(m, k, n_a=1):
        return 2 * -(-m // t["wm"]) * (-(-k // 64) * 64) * n_a

    def batched(batch, shared_a):
        a = torch.empty((1 if shared_a else batch, bk, bm), device="cuda")
        return ext.batched_workspace_floats(
            ti, a.expand(batch, bk, bm),
            torch.empty((batch, bk, bn), device="cuda"),
            torch.empty((batch, bn, bm), device="cuda"))

    # one tile, as a batch of one and as a ragged call
    assert batched(1, False) == want(bm, bk)
    assert ext.ragged_workspace_floats(ti, bm, bn, bk) == want(bm, bk)
    # one row past a band, K past a multiple of 64
    assert ext.ragged_workspace_floats(ti, bm + 1, bn + 1, 65) == \
        want(bm + 1, 65)
    assert want(bm + 1, 65) == 2 * (bm // t["wm"] + 1) * 128
    # a batch of 3, A shared (stride 0) and not
    assert batched(3, True) == want(bm, bk)
    assert batched(3, False) == want(bm, bk, 3)
