"""GPU tests of the transposed-operand forms of the ragged plain and
fused-ABFT SGEMM (ops.sgemm_ragged / ops.ft_sgemm_ragged with trans_a /
trans_b).

A transposed operand fills the same LDS panel as the untransposed one, so
the main check is exact: a transposed call on x.t().contiguous() must give
the bits of the plain ragged call on x, through the fast register path
(packed, aligned operands on whole blocks and panels) and through the
guarded one (4-byte-offset, odd-row-stride views).  With injection the
correction depends on the segment sums, so this covers the transposed
segment-sum kernel as well.  Shapes and conventions are those of
tests/test_gpu_ragged.py.
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
TRANS = {"TN": (True, False), "NT": (False, True), "TT": (True, True)}
MODES = ["plain", "fused", "fused_inject"]


def geom(tier):
    t = TILING[tier]
    return t["bm"], t["bn"], t.get("bkf", t["bk"])


def edge_shape(tier):
    bm, bn, bkf = geom(tier)
    return bm + 1, bn + 1, bkf + 1


def inject_shape(tier):
    bm, bn, bkf = geom(tier)
    return bm + 1, bn + 1, 6 * bkf + 5


def shapes(tier):
    bm, bn, bkf = geom(tier)
    return [edge_shape(tier), (3, 5, 7), (1, 1, 1),
            (2 * bm - 4, bn + 4, 5 * bkf + 4), (2 * bm, bn, 256)]


_cases = {}


def case(m, n, k):
    """Seeded packed (a, b, c0) of one shape, a (K, M) and b (K, N), made once
    and never written."""
    if (m, n, k) not in _cases:
        g = torch.Generator(device="cpu").manual_seed(7 * m + 3 * n + k)
        a = (torch.rand((k, m), generator=g) * 1.8 - 0.9).cuda()
        b = (torch.rand((k, n), generator=g) * 1.8 - 0.9).cuda()
        c0 = torch.randn((n, m), generator=g).cuda()
        _cases[(m, n, k)] = (a, b, c0)
    return _cases[(m, n, k)]


def lay(x, flag):
    """x as the call with that flag takes it: its transposed copy, or x."""
    return x.t().contiguous() if flag else x


def bordered(x, fill=NAN):
    """x copied into the view big[2:2+R, 3:3+C] of a parent filled with
    `fill`.  Returns (view, parent)."""
    r, c = x.shape
    big = torch.full((r + 5, c + 8), fill, device=x.device)
    view = big[2:2 + r, 3:3 + c]
    view.copy_(x)
    return view, big


def offset_strided(x):
    """x copied to a view whose base is 4 bytes past a 16-byte boundary and
    whose row stride is odd: nothing about it allows a 16-byte access."""
    r, c = x.shape
    ld = c + 1 + c % 2
    flat = torch.zeros(r * ld + 1, device=x.device)
    assert flat.data_ptr() % 16 == 0 and ld % 2 == 1
    view = flat.as_strided((r, c), (ld, 1), 1)
    view.copy_(x)
    return view


def run(tier, mode, a, b, c, ta=False, tb=False, alpha=ALPHA, beta=BETA,
        **kw):
    if mode == "plain":
        return ops.sgemm_ragged(tier, a, b, c, alpha, beta, trans_a=ta,
                                trans_b=tb)
    return ops.ft_sgemm_ragged(tier, a, b, c, alpha, beta,
                               inject=(mode == "fused_inject"), trans_a=ta,
                               trans_b=tb, **kw)


_untransposed = {}


def untransposed(tier, mode, m, n, k):
    """C of the plain ragged call on the packed case, computed once."""
    key = (tier, mode, m, n, k)
    if key not in _untransposed:
        a, b, c0 = case(m, n, k)
        _untransposed[key] = run(tier, mode, a, b, c0.clone())
    return _untransposed[key]


def site_counts(tier, m, n, k):
    """(n, m) fp64: predicted corrected injections per element of C."""
    v = torch.zeros((n, m), dtype=torch.float64)
    for e in predict_injected_events(tier, m, n, k, ragged=True):
        if e.i < m and e.j < n:
            v[e.j, e.i] += 1
    return v.cuda()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_bit_identical_to_untransposed(tier, trans, which, mode):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    ta, tb = TRANS[trans]
    m, n, k = shapes(tier)[which]
    a, b, c0 = case(m, n, k)
    want = untransposed(tier, mode, m, n, k)
    at, bt = lay(a, ta), lay(b, tb)
    c = c0.clone()
    run(tier, mode, at, bt, c, ta, tb)
    cs = offset_strided(c0)
    run(tier, mode, offset_strided(at), offset_strided(bt), cs, ta, tb)
    torch.cuda.synchronize()
    assert torch.equal(c, want), "packed transposed call differs"
    assert torch.equal(cs, want), "guarded-path transposed call differs"


@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_numerics(tier, trans):
    """Against the fp64 reference, so that the file does not rest on the
    other kernel alone: the edge shape (guarded path) and the aligned
    multi-panel one (fast path)."""
    ta, tb = TRANS[trans]
    for m, n, k in (shapes(tier)[0], shapes(tier)[4]):
        a, b, c0 = case(m, n, k)
        c = c0.clone()
        run(tier, "fused", lay(a, ta), lay(b, tb), c, ta, tb)
        torch.cuda.synchronize()
        eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                         eb.bound(a, b, c0, ALPHA, BETA, k),
                         f"{tier} {trans} {(m, n, k)}")


def check_window(cv, cbig, before, a, b, c0, k, extra, what):
    n, m = cv.shape
    assert torch.isfinite(cv).all(), what
    eb.assert_within(cv, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k) + extra, what)
    outside = torch.ones_like(cbig, dtype=torch.bool)
    outside[2:2 + n, 3:3 + m] = False
    assert torch.equal(cbig.view(torch.int32)[outside],
                       before.view(torch.int32)[outside]), what


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_guard_canaries(tier, trans, mode):
    """Operands, transposed ones included, are views of NaN-filled parents
    bordered in both directions: one out-of-range read in M, N or K makes
    the result non-finite; one out-of-range write changes C's parent."""
    ta, tb = TRANS[trans]
    m, n, k = edge_shape(tier)
    a, b, c0 = case(m, n, k)
    av, _ = bordered(lay(a, ta))
    bv, _ = bordered(lay(b, tb))
    cv, cbig = bordered(c0)
    before = cbig.clone()
    run(tier, mode, av, bv, cv, ta, tb)
    torch.cuda.synchronize()
    extra = (abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k)
             if mode == "fused_inject" else 0)
    check_window(cv, cbig, before, a, b, c0, k, extra,
                 f"{tier} {trans} {mode} canary")


def aligned_window(x, fill=NAN):
    """x copied into a view of a `fill`-filled parent whose base is 16-byte
    aligned and whose row stride is a multiple of 4 floats: the launch may
    use 16-byte reads on it, and the data right of each row is `fill`."""
    r, c = x.shape
    ld = (c + 8 + 3) // 4 * 4
    big = torch.full((r + 8, ld), fill, device=x.device)
    view = big[4:4 + r, 4:4 + c]
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    view.copy_(x)
    return view


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_fast_path_stops_at_k(tier, trans, mode):
    """16-byte-aligned base, ld % 4 == 0, whole blocks, but K % 4 != 0: the
    fast path is allowed on the whole panels only.  A 16-byte read across K
    in the last panel would pick up the NaN right of the row."""
    ta, tb = TRANS[trans]
    bm, bn, bkf = geom(tier)
    m, n, k = 2 * bm, bn, 2 * bkf + 1
    assert k % 4 != 0
    a, b, c0 = case(m, n, k)
    av = aligned_window(lay(a, ta))
    bv = aligned_window(lay(b, tb))
    cv, cbig = bordered(c0)
    before = cbig.clone()
    run(tier, mode, av, bv, cv, ta, tb)
    torch.cuda.synchronize()
    extra = (abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k)
             if mode == "fused_inject" else 0)
    check_window(cv, cbig, before, a, b, c0, k, extra,
                 f"{tier} {trans} {mode} aligned K tail")


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_beta_zero_never_reads_c(tier, trans, mode):
    ta, tb = TRANS[trans]
    m, n, k = edge_shape(tier)
    a, b, _ = case(m, n, k)
    av, _ = bordered(lay(a, ta))
    bv, _ = bordered(lay(b, tb))
    cv, _ = bordered(torch.full((n, m), NAN, device="cuda"))
    run(tier, mode, av, bv, cv, ta, tb, ALPHA, 0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(cv).all()
    e = eb.bound(a, b, None, ALPHA, 0.0, k)
    if mode == "fused_inject":
        e = e + abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k)
    eb.assert_within(cv, eb.ref64(a, b, None, ALPHA, 0.0), e,
                     f"{tier} {trans} {mode} beta=0")


@pytest.mark.parametrize("layout", ["packed", "nan_bordered"])
@pytest.mark.parametrize("trans", ["TN", "TT"])
@pytest.mark.parametrize("tier", TIERS)
def test_edge_tile_checksums_consistent(tier, trans, layout):
    """No injection and a tight tau, A transposed: were the transposed
    segment sums of an edge band taken over anything but its real rows and
    k, the verify would trip."""
    ta, tb = TRANS[trans]
    m, n, k = inject_shape(tier)
    a, b, c0 = case(m, n, k)
    at, bt = lay(a, ta), lay(b, tb)
    if layout == "packed":
        c = c0.clone()
    else:
        at, bt, c = bordered(at)[0], bordered(bt)[0], bordered(c0)[0]
    rep = FaultReport()
    ops.ft_sgemm_ragged(tier, at, bt, c, ALPHA, BETA, inject=False, tau=100.0,
                        report=rep, trans_a=ta, trans_b=tb)
    r = rep.read()
    assert (r.tripped, r.n_events, r.corrected, r.uncorrected,
            r.unlocated) == (0, 0, 0, 0, 0)
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k),
                     f"{tier} {trans} tau=100")


@pytest.mark.parametrize("trans", ["TN", "TT"])
@pytest.mark.parametrize("tier", TIERS)
def test_stale_workspace(tier, trans):
    """Best effort, as in tests/test_gpu_ragged.py: a NaN-filled tensor of
    the workspace's size is freed right before the call.  With K = bkf + 1
    the last panel and the strip window read segment sums well past K; the
    guarantee is the transposed segment-sum kernel's zero fill of
    [K, sstr)."""
    ta, tb = TRANS[trans]
    m, n, k = edge_shape(tier)
    a, b, c0 = case(m, n, k)
    at, bt = lay(a, ta), lay(b, tb)
    nws = ops._require_ext().ragged_workspace_floats(ops.tier_index(tier),
                                                     m, n, k)
    stale = torch.full((nws,), NAN, device="cuda")
    del stale
    rep = FaultReport()
    c = c0.clone()
    ops.ft_sgemm_ragged(tier, at, bt, c, ALPHA, BETA, inject=False, tau=100.0,
                        report=rep, trans_a=ta, trans_b=tb)
    r = rep.read()
    assert torch.isfinite(c).all()
    assert (r.tripped, r.n_events, r.unlocated) == (0, 0, 0)
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k),
                     f"{tier} {trans} stale ws")


@pytest.mark.parametrize("trans", TRANS)
@pytest.mark.parametrize("tier", TIERS)
def test_inject_correct_report(tier, trans):
    """Transposition does not move a fault: the events are the ragged
    kernel's predicted ones, all corrected, and C does not depend on the
    report."""
    ta, tb = TRANS[trans]
    m, n, k = inject_shape(tier)
    a, b, c0 = case(m, n, k)
    at, bt = lay(a, ta), lay(b, tb)
    want = predict_injected_events(tier, m, n, k, ragged=True)
    assert len(want) == 4 * 7
    rep = FaultReport()
    c = c0.clone()
    ops.ft_sgemm_ragged(tier, at, bt, c, ALPHA, BETA, inject=True, report=rep,
                        trans_a=ta, trans_b=tb)
    r = rep.read()
    key = lambda e: (e.i, e.j, e.k_begin, e.k_end, e.status)  # noqa: E731
    assert sorted(map(key, r.events)) == sorted(map(key, want))
    assert r.n_events == len(want) and r.corrected == r.n_events
    assert r.uncorrected == r.unlocated == r.dropped == 0
    e = (eb.bound(a, b, c0, ALPHA, BETA, k) +
         abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k))
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA), e,
                     f"{tier} {trans} inject")
    c2 = c0.clone()
    ops.ft_sgemm_ragged(tier, at, bt, c2, ALPHA, BETA, inject=True,
                        trans_a=ta, trans_b=tb)
    torch.cuda.synchronize()
    assert torch.equal(c, c2), "C depends on the report"


@pytest.mark.parametrize("trans", TRANS)
def test_binding_refuses_a_short_leading_dimension(trans):
    """A transposed operand's leading dimension is held against K, by the
    launch rules themselves (the binding is called directly: ragged_layout
    would refuse first)."""
    ta, tb = TRANS[trans]
    m, n, k = 8, 9, 12
    a, b, c0 = case(m, n, k)
    at, bt = lay(a, ta), lay(b, tb)
    short = lambda x: x.as_strided(x.shape, (k - 1, 1))  # noqa: E731
    c = c0.clone()
    before = c.clone()
    ext = ops._require_ext()
    with pytest.raises(RuntimeError, match="leading dimension"):
        ext.sgemm_ragged(ops.tier_index("small"), False, False,
                         short(at) if ta else at, short(bt) if tb else bt, c,
                         ALPHA, BETA, 0.0, 0.0, 20, trans_a=ta, trans_b=tb)
    torch.cuda.synchronize()
    assert torch.equal(c, before)
    # a row stride of exactly K passes, and M (or N) is not what it is held to
    assert k > m and k > n
    run("small", "plain", at, bt, c, ta, tb)
    with pytest.raises(ValueError, match="overlap"):
        ops.sgemm_ragged("small", short(at) if ta else at,
                         short(bt) if tb else bt, c, trans_a=ta, trans_b=tb)
