"""GPU tests of the ragged plain and fused-ABFT SGEMM (ops.sgemm_ragged /
ops.ft_sgemm_ragged): any M, N, K, row-strided operands, 4-byte alignment.

Shapes are the smallest at which the kernel can go wrong, per tier with
tile (bm, bn) and fused panel depth bkf: one row, one column and one k past
a tile (a 2 x 2 grid whose three edge blocks are almost all padding, and a
second panel holding a single k), a shape smaller than any tile, 1 x 1 x 1,
and an aligned multi-panel shape that takes the 16-byte staging path on its
full blocks.  Numerics are checked against the fp64 reference within the
derived bound of utils/errbound.py; a corrected fault site gets the
project's |alpha| * 1e-2 on top (FAULT_TOL of tests/test_gpu_threshold.py).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING
from ft_sgemm_amd.ops.fault_report import FaultReport, predict_injected_events
from ft_sgemm_amd.utils import errbound as eb

ALPHA, BETA = 1.5, -0.5
FAULT_TOL = 1e-2  # per corrected fault, tests/test_gpu_threshold.py
NAN = float("nan")


def geom(tier):
    t = TILING[tier]
    return t["bm"], t["bn"], t.get("bkf", t["bk"])


def edge_shape(tier):
    bm, bn, bkf = geom(tier)
    return bm + 1, bn + 1, bkf + 1


def inject_shape(tier):
    bm, bn, bkf = geom(tier)
    return bm + 1, bn + 1, 6 * bkf + 5


_cases = {}


def case(m, n, k):
    """Seeded packed (a, b, c0) of one shape, made once and never written."""
    if (m, n, k) not in _cases:
        g = torch.Generator(device="cpu").manual_seed(7 * m + 3 * n + k)
        a = (torch.rand((k, m), generator=g) * 1.8 - 0.9).cuda()
        b = (torch.rand((k, n), generator=g) * 1.8 - 0.9).cuda()
        c0 = torch.randn((n, m), generator=g).cuda()
        _cases[(m, n, k)] = (a, b, c0)
    return _cases[(m, n, k)]


def bordered(x, fill=NAN):
    """x copied into the view big[2:2+R, 3:3+C] of a parent filled with
    `fill`.  Returns (view, parent)."""
    r, c = x.shape
    big = torch.full((r + 5, c + 8), fill, device=x.device)
    view = big[2:2 + r, 3:3 + c]
    view.copy_(x)
    return view, big


def run(tier, mode, a, b, c, alpha=ALPHA, beta=BETA, **kw):
    if mode == "plain":
        return ops.sgemm_ragged(tier, a, b, c, alpha, beta)
    return ops.ft_sgemm_ragged(tier, a, b, c, alpha, beta,
                               inject=(mode == "fused_inject"), **kw)


def site_counts(tier, m, n, k):
    """(n, m) fp64: predicted corrected injections per element of C."""
    v = torch.zeros((n, m), dtype=torch.float64)
    for e in predict_injected_events(tier, m, n, k, ragged=True):
        if e.i < m and e.j < n:
            v[e.j, e.i] += 1
    return v.cuda()


def numerics_shapes(tier):
    bm, bn, bkf = geom(tier)
    return [edge_shape(tier), (3, 5, 7), (1, 1, 1),
            (2 * bm - 4, bn + 4, 5 * bkf + 4)]


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("tier", TIERS)
def test_numerics(tier, which, mode):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    m, n, k = numerics_shapes(tier)[which]
    a, b, c0 = case(m, n, k)
    c = c0.clone()
    run(tier, mode, a, b, c)
    torch.cuda.synchronize()
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k),
                     f"{tier} {mode} {(m, n, k)}")


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_guard_canaries(tier, mode):
    """Operands are views of NaN-filled parents: one out-of-range read in M,
    N or K makes the result non-finite; one out-of-range write changes the
    bits of C's parent."""
    m, n, k = edge_shape(tier)
    a, b, c0 = case(m, n, k)
    av, _ = bordered(a)
    bv, _ = bordered(b)
    cv, cbig = bordered(c0)
    before = cbig.clone()
    run(tier, mode, av, bv, cv)
    torch.cuda.synchronize()
    assert torch.isfinite(cv).all()
    e = eb.bound(a, b, c0, ALPHA, BETA, k)
    if mode == "fused_inject":
        e = e + abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k)
    eb.assert_within(cv, eb.ref64(a, b, c0, ALPHA, BETA), e,
                     f"{tier} {mode} canary")
    outside = torch.ones_like(cbig, dtype=torch.bool)
    outside[2:2 + n, 3:3 + m] = False
    assert torch.equal(cbig.view(torch.int32)[outside],
                       before.view(torch.int32)[outside])


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_beta_zero_never_reads_c(tier, mode):
    m, n, k = edge_shape(tier)
    a, b, _ = case(m, n, k)
    av, _ = bordered(a)
    bv, _ = bordered(b)
    cv, _ = bordered(torch.full((n, m), NAN, device="cuda"))
    run(tier, mode, av, bv, cv, ALPHA, 0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(cv).all()
    e = eb.bound(a, b, None, ALPHA, 0.0, k)
    if mode == "fused_inject":
        e = e + abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k)
    eb.assert_within(cv, eb.ref64(a, b, None, ALPHA, 0.0), e,
                     f"{tier} {mode} beta=0")


def offset_strided(x):
    """x copied to a view whose base is 4 bytes past a 16-byte boundary and
    whose row stride is no multiple of 4 floats: nothing about it allows a
    16-byte access."""
    r, c = x.shape
    assert c % 4 == 0
    ld = c + 3
    flat = torch.zeros(r * ld + 1, device=x.device)
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided((r, c), (ld, 1), 1)
    view.copy_(x)
    return view


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", TIERS)
def test_bit_identical_to_tiled(tier, mode, monkeypatch):
    """On a shape the tile divides the ragged kernel is the tiled kernel:
    same bits, through the 16-byte staging path (packed operands) and
    through the guarded one (offset, odd-stride views of the same data)."""
    monkeypatch.setenv("FT_SGEMM_STREAMK", "0")
    bm, bn, _ = geom(tier)
    m, n, k = 2 * bm, bn, 256
    a, b, c0 = case(m, n, k)
    want = c0.clone()
    if mode == "plain":
        ops.sgemm(tier, a, b, want, ALPHA, BETA)
    else:
        ops.ft_sgemm(tier, a, b, want, ALPHA, BETA, inject=True)
    c = c0.clone()
    run(tier, mode, a, b, c)
    cs = offset_strided(c0)
    run(tier, mode, offset_strided(a), offset_strided(b), cs)
    torch.cuda.synchronize()
    assert torch.equal(c, want), "packed ragged differs from tiled"
    assert torch.equal(cs, want), "guarded-path ragged differs from tiled"


@pytest.mark.parametrize("layout", ["packed", "nan_bordered"])
@pytest.mark.parametrize("tier", TIERS)
def test_inject_correct_report(tier, layout):
    m, n, k = inject_shape(tier)
    a, b, c0 = case(m, n, k)
    if layout == "packed":
        av, bv, mk = a, b, lambda: c0.clone()
    else:
        av, bv = bordered(a)[0], bordered(b)[0]
        mk = lambda: bordered(c0)[0]  # noqa: E731
    want = predict_injected_events(tier, m, n, k, ragged=True)
    assert len(want) == 4 * 7
    rep = FaultReport()
    c = mk()
    ops.ft_sgemm_ragged(tier, av, bv, c, ALPHA, BETA, inject=True, report=rep)
    r = rep.read()
    key = lambda e: (e.i, e.j, e.k_begin, e.k_end, e.status)  # noqa: E731
    assert sorted(map(key, r.events)) == sorted(map(key, want))
    assert r.n_events == len(want) and r.corrected == r.n_events
    assert r.uncorrected == r.unlocated == r.dropped == 0
    e = (eb.bound(a, b, c0, ALPHA, BETA, k) +
         abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k))
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA), e,
                     f"{tier} {layout} inject")
    c2 = mk()
    ops.ft_sgemm_ragged(tier, av, bv, c2, ALPHA, BETA, inject=True)
    torch.cuda.synchronize()
    assert torch.equal(c, c2), "C depends on the report"


@pytest.mark.parametrize("layout", ["packed", "nan_bordered"])
@pytest.mark.parametrize("tier", TIERS)
def test_edge_tile_checksums_consistent(tier, layout):
    """No injection and a tight tau: were an edge tile's checksums taken over
    anything but its real rows, columns and k, its verify would trip."""
    m, n, k = inject_shape(tier)
    a, b, c0 = case(m, n, k)
    if layout == "packed":
        av, bv, c = a, b, c0.clone()
    else:
        av, bv, c = bordered(a)[0], bordered(b)[0], bordered(c0)[0]
    rep = FaultReport()
    ops.ft_sgemm_ragged(tier, av, bv, c, ALPHA, BETA, inject=False, tau=100.0,
                        report=rep)
    r = rep.read()
    assert (r.tripped, r.n_events, r.corrected, r.uncorrected,
            r.unlocated) == (0, 0, 0, 0, 0)
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k), f"{tier} tau=100")


@pytest.mark.parametrize("tier", TIERS)
def test_stale_workspace(tier):
    """Best effort: a NaN-filled tensor of the workspace's size is freed
    right before the call, so the caching allocator is likely (not certain)
    to hand that block to the fused call.  With K = bkf + 1 the last panel
    and the strip window read segment sums well past K.  The actual
    guarantee is the zero fill of [K, sstr) in the ragged segment-sum
    kernel; this test only makes a missing one likely to show."""
    m, n, k = edge_shape(tier)
    a, b, c0 = case(m, n, k)
    nws = ops._require_ext().ragged_workspace_floats(ops.tier_index(tier),
                                                     m, n, k)
    stale = torch.full((nws,), NAN, device="cuda")
    del stale
    rep = FaultReport()
    c = c0.clone()
    ops.ft_sgemm_ragged(tier, a, b, c, ALPHA, BETA, inject=False, report=rep)
    r = rep.read()
    assert torch.isfinite(c).all()
    assert (r.tripped, r.n_events, r.unlocated) == (0, 0, 0)
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k), f"{tier} stale ws")


@pytest.mark.parametrize("shape", [(257, 129, 65), (100, 100, 100)])
def test_auto_routing(shape):
    m, n, k = shape
    assert ops.choose_tier(m, n, k) is None
    tier = ops.choose_tier(m, n, k, ragged=True)
    a, b, c0 = case(m, n, k)
    ref = eb.ref64(a, b, c0, ALPHA, BETA)
    rep = FaultReport()
    c = c0.clone()
    ops.ft_sgemm_auto(a, b, c, ALPHA, BETA, report=rep, misfit="ragged")
    r = rep.read()
    assert r.corrected > 0 and r.uncorrected == r.unlocated == 0
    e = (eb.bound(a, b, c0, ALPHA, BETA, k) +
         abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k))
    eb.assert_within(c, ref, e, f"auto ragged {shape}")
    # the default routing is today's: rocBLAS + offline chain, no report
    rep = FaultReport()
    c = c0.clone()
    ops.ft_sgemm_auto(a, b, c, ALPHA, BETA, report=rep)
    r = rep.read()
    assert (r.tripped, r.n_events) == (0, 0)
    assert torch.isfinite(c).all()


def test_tiled_entry_still_refuses_a_misfit():
    a, b, c0 = case(257, 129, 65)
    with pytest.raises(RuntimeError):
        ops.sgemm("huge", a, b, c0.clone())
