"""GPU tests of the strided-batched ragged plain and fused-ABFT SGEMM
(ops.sgemm_ragged_batched / ops.ft_sgemm_ragged_batched).

Only the kernel's prologue knows about the batch, so the main check is exact:
entry i of a batched launch must have the bits of the single ragged launch on
the views a[i], b[i], c[i], for every tier, mode and transpose combination.
One shape rule per tier: M = bm + 1, N = 2*bn + 3, K = 133, batch 3 — edge
tiles in both directions, more blocks in y than in x, two 64-k strip windows
plus a K tail, and odd packed entry sizes, so that entry 1 is misaligned where
entry 0 is aligned (the per-entry fast bits).  torch.bmm is the independent
reference, at the tolerance of tests/test_gpu_kernels.py.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING
from ft_sgemm_amd.ops.fault_report import predict_injected_events

ABS_TOL = 1e-2  # tests/test_gpu_kernels.py
REL_TOL = 1e-2
BATCH, K = 3, 133
ALPHA, BETA = 1.25, -1.5
NAN = float("nan")
SENTINEL = -12345.0
MODES = ["plain", "fused", "fused_inject"]
TRANS = {"NN": (False, False), "TN": (True, False), "NT": (False, True),
         "TT": (True, True)}
FUSED_TRANS_TIERS = ("huge", "tall", "small")


def shape(tier):
    t = TILING[tier]
    return t["bm"] + 1, 2 * t["bn"] + 3, K


def check(ref, got):
    diff = (ref - got).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


def run_single(tier, mode, a, b, c, ta=False, tb=False, **kw):
    if mode == "plain":
        return ops.sgemm_ragged(tier, a, b, c, ALPHA, BETA, trans_a=ta,
                                trans_b=tb)
    return ops.ft_sgemm_ragged(tier, a, b, c, ALPHA, BETA,
                               inject=(mode == "fused_inject"), trans_a=ta,
                               trans_b=tb, **kw)


def run_batched(tier, mode, a, b, c, ta=False, tb=False, **kw):
    if mode == "plain":
        return ops.sgemm_ragged_batched(tier, a, b, c, ALPHA, BETA,
                                        trans_a=ta, trans_b=tb)
    return ops.ft_sgemm_ragged_batched(tier, a, b, c, ALPHA, BETA,
                                       inject=(mode == "fused_inject"),
                                       trans_a=ta, trans_b=tb, **kw)


_operands = {}


def operands(tier, dims=None):
    """Seeded packed (a, b, c0), a (B, K, M), b (B, K, N), c0 (B, N, M) with a
    C that differs per entry; made once and never written to."""
    m, n, k = dims or shape(tier)
    if (m, n, k) not in _operands:
        g = torch.Generator(device="cpu").manual_seed(7 * m + 3 * n + k)
        a = (torch.rand((BATCH, k, m), generator=g) * 1.8 - 0.9).cuda()
        b = (torch.rand((BATCH, k, n), generator=g) * 1.8 - 0.9).cuda()
        c0 = torch.randn((BATCH, n, m), generator=g).cuda()
        _operands[(m, n, k)] = (a, b, c0)
    return _operands[(m, n, k)]


def lay(x, flag):
    """x as the call with that flag takes it: its transposed copy, or x."""
    return x.transpose(-1, -2).contiguous() if flag else x


_packed = {}


def packed(tier, mode, trans="NN"):
    """C of the batched launch on the packed operands, computed once."""
    key = (tier, mode, trans)
    if key not in _packed:
        ta, tb = TRANS[trans]
        a, b, c0 = operands(tier)
        _packed[key] = run_batched(tier, mode, lay(a, ta), lay(b, tb),
                                   c0.clone(), ta, tb)
        torch.cuda.synchronize()
    return _packed[key]


@pytest.mark.parametrize("tier,trans,mode", [
    (tier, trans, mode) for tier in TIERS for trans in TRANS for mode in MODES
    if mode == "plain" or trans == "NN" or tier in FUSED_TRANS_TIERS])
def test_bit_identical_to_single_launches(tier, trans, mode):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    ta, tb = TRANS[trans]
    a, b, c0 = operands(tier)
    at, bt = lay(a, ta), lay(b, tb)
    assert at[1].data_ptr() % 16 and bt[1].data_ptr() % 16
    c = packed(tier, mode, trans)
    want = c0.clone()
    for i in range(BATCH):
        run_single(tier, mode, at[i], bt[i], want[i], ta, tb)
    torch.cuda.synchronize()
    for i in range(BATCH):
        assert torch.equal(c[i], want[i]), (
            f"entry {i}: {int((c[i] != want[i]).sum())} elements differ from "
            f"the single launch")
    check(ops.torch_reference_batched(a, b, c0, ALPHA, BETA), c)


def padded(x, fill, offset=0):
    """x (B, R, C) copied into a `fill`-filled flat buffer as a view with a
    leading dimension of C + 3, a gap of 5 floats after every entry and its
    base `offset` floats in.  Returns (view, flat, mask of everything that is
    not the view)."""
    bsz, r, c = x.shape
    ld = c + 3
    step = r * ld + 5
    size = (bsz, r, c), (step, ld, 1), offset
    flat = torch.full((offset + bsz * step,), fill, device=x.device)
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided(*size)
    view.copy_(x)
    mask = torch.ones_like(flat, dtype=torch.bool)
    mask.as_strided(*size).fill_(False)
    return view, flat, mask


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("trans", ["NN", "TT"])
@pytest.mark.parametrize("tier", TIERS)
def test_padding_is_never_touched(tier, trans, mode, offset):
    """Row padding and batch gaps of A and B hold NaN, those of C a sentinel:
    one read outside an entry makes the result non-finite, one write outside
    changes a sentinel."""
    ta, tb = TRANS[trans]
    a, b, c0 = operands(tier)
    ap, _, _ = padded(lay(a, ta), NAN, offset)
    bp, _, _ = padded(lay(b, tb), NAN, offset)
    cp, cflat, cmask = padded(c0, SENTINEL, offset)
    m, n, _ = shape(tier)
    got = ops.ragged_batched_layout(ap, bp, cp, ta, tb)
    assert got[6] == m + 3 and got[9] == n * (m + 3) + 5
    run_batched(tier, mode, ap, bp, cp, ta, tb)
    torch.cuda.synchronize()
    assert torch.equal(cp, packed(tier, mode, trans))
    assert int(cmask.sum()) == cflat.numel() - c0.numel()
    assert bool((cflat[cmask] == SENTINEL).all()), "C's padding was written"


@pytest.mark.parametrize("tier", TIERS)
def test_shared_operands(tier):
    """expand()ed (stride 0) and 2-D operands, fused with injection, equal
    the run on materialised copies; a shared A is encoded once and asks for
    one matrix's workspace."""
    a, b, c0 = operands(tier)
    m, n, k = shape(tier)
    ext = ops._require_ext()
    ti = ops.tier_index(tier)
    mode = "fused_inject"

    a_sh = a[1].expand(BATCH, k, m)
    assert a_sh.stride(0) == 0
    a_mat = a_sh.contiguous()
    c_mat = run_batched(tier, mode, a_mat, b, c0.clone())
    for a_in in (a_sh, a[1]):
        c = run_batched(tier, mode, a_in, b, c0.clone())
        torch.cuda.synchronize()
        assert torch.equal(c, c_mat)
    check(ops.torch_reference_batched(a[1], b, c0, ALPHA, BETA), c_mat)
    one = ext.ragged_batched_workspace_floats(ti, a[:1], b[:1], c0[:1])
    assert one == ext.ragged_workspace_floats(ti, m, n, k) > 0
    assert ext.ragged_batched_workspace_floats(ti, a_sh, b, c0) == one
    assert ext.ragged_batched_workspace_floats(ti, a_mat, b, c0) == BATCH * one

    # a shared transposed a
    at = a[1].t().contiguous()
    for a_in in (at, at.expand(BATCH, m, k)):
        c = run_batched(tier, mode, a_in, b, c0.clone(), True, False)
        torch.cuda.synchronize()
        assert torch.equal(c, c_mat)
    assert ext.ragged_batched_workspace_floats(
        ti, at.expand(BATCH, m, k), b, c0, True, False) == one

    b_sh = b[2].expand(BATCH, k, n)
    c_mat = run_batched(tier, mode, a, b_sh.contiguous(), c0.clone())
    for b_in in (b_sh, b[2]):
        c = run_batched(tier, mode, a, b_in, c0.clone())
        torch.cuda.synchronize()
        assert torch.equal(c, c_mat)
    check(ops.torch_reference_batched(a, b[2], c0, ALPHA, BETA), c_mat)


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_interleaved_c(tier, mode):
    """C's entries as heads inside a (T, H*D) tensor: entry h is the column
    block [h*D, (h+1)*D) of every row.  Two spare columns per row hold a
    sentinel."""
    a, b, c0 = operands(tier)
    m, n, _ = shape(tier)
    whole = torch.full((n, BATCH * m + 2), SENTINEL, device="cuda")
    cv = whole[:, :BATCH * m].view(n, BATCH, m).permute(1, 0, 2)
    assert cv.stride() == (m, BATCH * m + 2, 1)
    cv.copy_(c0)
    assert ops.ragged_batched_layout(a, b, cv)[6:] == (
        BATCH * m + 2, K * m, K * n, m)
    run_batched(tier, mode, a, b, cv)
    torch.cuda.synchronize()
    assert torch.equal(cv, packed(tier, mode))
    assert bool((whole[:, BATCH * m:] == SENTINEL).all())


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_aligned_divisible_shape_is_the_tiled_batch(tier, mode):
    t = TILING[tier]
    dims = (2 * t["bm"], 3 * t["bn"], 128)
    a, b, c0 = operands(tier, dims)
    c = run_batched(tier, mode, a, b, c0.clone())
    if mode == "plain":
        want = ops.sgemm_batched(tier, a, b, c0.clone(), ALPHA, BETA)
    else:
        want = ops.ft_sgemm_batched(tier, a, b, c0.clone(), ALPHA, BETA,
                                    inject=True)
    torch.cuda.synchronize()
    assert torch.equal(c, want)


@pytest.mark.parametrize("tier", ["huge", "tall", "small"])
def test_report_per_entry(tier):
    """Every entry logs its own injections, padded victims included, into its
    own slot."""
    a, b, c0 = operands(tier)
    m, n, k = shape(tier)
    expect = predict_injected_events(tier, m, n, k, ragged=True)
    assert any(e.i >= m or e.j >= n for e in expect), "no padded victim"
    rep = ops.BatchedFaultReport(BATCH)
    c = run_batched(tier, "fused_inject", a, b, c0.clone(), report=rep)
    got = rep.read()
    assert torch.equal(c, packed(tier, "fused_inject")), (
        "C changed with a report attached")
    key = lambda e: (e.i, e.j, e.k_begin, e.k_end, e.status)  # noqa: E731
    assert len(got) == BATCH
    for i, r in enumerate(got):
        assert sorted(map(key, r.events)) == sorted(map(key, expect)), i
        assert r.n_events == len(expect) and r.corrected == len(expect), i
        assert r.uncorrected == r.unlocated == r.dropped == 0, i
    rep.raise_if_uncorrected()
    with pytest.raises(ValueError, match="report holds"):
        run_batched(tier, "fused_inject", a, b, c0.clone(),
                    report=ops.BatchedFaultReport(BATCH + 1))


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", ["medium", "huge"])
def test_smallest_cases(tier, mode):
    g = torch.Generator(device="cpu").manual_seed(5)
    a, b, c0 = (torch.randn((2, 1, 1), generator=g).cuda() for _ in range(3))
    c = run_batched(tier, mode, a, b, c0.clone())
    torch.cuda.synchronize()
    check(ops.torch_reference_batched(a, b, c0, ALPHA, BETA), c)
    # a batch of one is the single ragged launch
    a, b, c0 = operands(tier)
    c_b = run_batched(tier, mode, a[:1], b[:1], c0[:1].clone())
    c_s = run_single(tier, mode, a[0], b[0], c0[0].clone())
    torch.cuda.synchronize()
    assert torch.equal(c_b[0], c_s)


# ---- the launch rules, through the raw binding ----------------------------
# ragged_batched_layout would refuse each of these first; gemm_args_error and
# the binding's own checks must refuse them too, with nothing launched.

def _rej_operands():
    m, n, k = 8, 9, 12
    g = torch.Generator(device="cpu").manual_seed(99)
    rand = lambda *s: torch.rand(s, generator=g).cuda()  # noqa: E731
    c_flat = rand(BATCH * k * n)  # room for every strided view made of it
    return dict(a=rand(BATCH, k, m), b=rand(BATCH, k, n), c_flat=c_flat,
                c=c_flat[:BATCH * n * m].view(BATCH, n, m), abft=False,
                log=(None, None))


def _overlap_disjoint():
    d = _rej_operands()
    _, n, m = d["c"].shape
    d["c"] = d["c_flat"].as_strided((BATCH, n, m), (n * m - 1, m, 1))
    return d


def _overlap_interleaved():
    d = _rej_operands()
    _, n, m = d["c"].shape
    d["c"] = d["c_flat"].as_strided((BATCH, n, m), (m - 1, BATCH * m, 1))
    return d


def _short_row(which):
    def build():
        d = _rej_operands()
        bsz, rows, width = d[which].shape
        d[which] = d["c_flat"].as_strided((bsz, rows, width),
                                          (rows * width, width - 1, 1))
        return d
    return build


def _batch_mismatch():
    d = _rej_operands()
    d["a"] = d["a"][:2]
    return d


def _bad_log():
    d = _rej_operands()
    d["abft"] = True
    d["log"] = (torch.full((5,), 7, dtype=torch.int32, device="cuda"),
                torch.full((BATCH, 4, 8), 7, dtype=torch.int32,
                           device="cuda"))
    return d


REJECTIONS = {
    "overlap_disjoint": ("C entries overlap", _overlap_disjoint),
    "overlap_interleaved": ("C entries overlap", _overlap_interleaved),
    "short_row_a": ("shorter than", _short_row("a")),
    "short_row_c": ("shorter than", _short_row("c")),
    "batch_mismatch": ("one batch size", _batch_mismatch),
    "log_shape": ("fault-log counters must", _bad_log),
}


@pytest.mark.parametrize("case", list(REJECTIONS))
def test_binding_rejects_bad_launches(case):
    text, build = REJECTIONS[case]
    d = build()
    watched = [d["c_flat"]] + [x for x in d["log"] if x is not None]
    before = [x.clone() for x in watched]
    with pytest.raises(RuntimeError, match=text):
        ops._require_ext().sgemm_ragged_batched(
            ops.tier_index("medium"), d["abft"], False, d["a"], d["b"],
            d["c"], 1.0, 0.0, 0.0, 0.0, 20, *d["log"])
    torch.cuda.synchronize()
    for x, x0 in zip(watched, before):
        assert torch.equal(x, x0), "a rejected call wrote to its tensors"
