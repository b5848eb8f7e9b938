"""GPU tests of the ragged stream-K launch (ops.sgemm_ragged /
ops.ft_sgemm_ragged with streamk=): any M, N, K, row-strided and transposed
operands, caller-owned partials.

Shapes, per tier with tile (bm, bn): one row and one column past a tile and a
K of three (two) whole 64-k units plus five, so that every tile's last unit is
short.  CASES lists the (shape, grid) pairs; tests/test_ragged_streamk_cpu.py
asserts that together they hold a fully-owned tile, a tile split across two
workgroups, one split across three or more with a workgroup wholly inside it,
and a workgroup with head + full tile + tail.  Numerics are checked against
the fp64 reference within the bound of utils/errbound.py, which holds for any
summation order and so needs no widening for the slot sum; a corrected fault
site gets the project's |alpha| * 1e-2 on top.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TILING
from ft_sgemm_amd.ops.fault_report import FaultReport, predict_injected_events
from ft_sgemm_amd.utils import errbound as eb

SK_TIERS = ("large", "huge")
ALPHA, BETA = 1.5, -0.5
FAULT_TOL = 1e-2  # per corrected fault, tests/test_gpu_threshold.py
NAN = float("nan")


def geom(tier):
    t = TILING[tier]
    return t["bm"], t["bn"], t.get("bkf", t["bk"])


def split_cases(tier):
    """(shape, grid) pairs with tiles shared between workgroups."""
    bm, bn, _ = geom(tier)
    s4 = (bm + 1, bn + 1, 3 * 64 + 5)      # 4 tiles x 4 units
    s6 = (2 * bm + 1, bn + 1, 2 * 64 + 5)  # 6 tiles x 3 units
    return [(s4, 1), (s4, 3), (s4, 5), (s4, 16), (s6, 4)]


def CASES(tier):
    return split_cases(tier) + [((3, 5, 7), 2), ((1, 1, 1), 4)]


N_CASES = 7

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


def run(tier, mode, a, b, c, alpha=ALPHA, beta=BETA, **kw):
    if mode == "plain":
        return ops.sgemm_ragged(tier, a, b, c, alpha, beta, **kw)
    return ops.ft_sgemm_ragged(tier, a, b, c, alpha, beta,
                               inject=(mode == "fused_inject"), **kw)


def bits(x):
    return x.contiguous().view(torch.int32)


def site_counts(tier, m, n, k, grid, vw=20):
    """(n, m) fp64: predicted corrected injections per element of C."""
    v = torch.zeros((n, m), dtype=torch.float64)
    for e in predict_injected_events(tier, m, n, k, vw, ragged=True,
                                     streamk_grid=grid):
        if e.i < m and e.j < n:
            v[e.j, e.i] += 1
    return v.cuda()


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("which", range(N_CASES))
@pytest.mark.parametrize("tier", SK_TIERS)
def test_numerics(tier, which, mode):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    (m, n, k), grid = CASES(tier)[which]
    a, b, c0 = case(m, n, k)
    c = c0.clone()
    run(tier, mode, a, b, c, streamk=grid)
    torch.cuda.synchronize()
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k),
                     f"{tier} {mode} {(m, n, k)} grid {grid}")


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("tier", SK_TIERS)
def test_bit_composition(tier, which, mode):
    """alpha = 1, beta = 0: every tile is, bit for bit, the left-to-right
    fp32 sum of the classic launch's results on the K slices of the tile's
    segments, in workgroup order."""
    (m, n, k), grid = split_cases(tier)[which]
    bm, bn, _ = geom(tier)
    a, b, _ = case(m, n, k)
    got = torch.empty((n, m), device="cuda")
    run(tier, mode, a, b, got, 1.0, 0.0, streamk=grid)
    slices = {}

    def classic(w_lo, w_hi):
        if (w_lo, w_hi) not in slices:
            lo, hi = 64 * w_lo, min(k, 64 * w_hi)
            out = torch.empty((n, m), device="cuda")
            run(tier, mode, a[lo:hi], b[lo:hi], out, 1.0, 0.0)
            slices[(w_lo, w_hi)] = out
        return slices[(w_lo, w_hi)]

    per_tile = {}
    for segs in ops.ragged_streamk_partition(tier, m, n, k, grid)[0]:
        for tile, bx, by, w_lo, w_hi, _ in segs:
            per_tile.setdefault((bx, by), []).append((w_lo, w_hi))
    want = torch.empty_like(got)
    for (bx, by), segs in per_tile.items():
        win = (slice(by * bn, min(n, (by + 1) * bn)),
               slice(bx * bm, min(m, (bx + 1) * bm)))
        s = classic(*segs[0])[win].clone()
        for seg in segs[1:]:
            s = s + classic(*seg)[win]
        want[win] = s
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("tier", SK_TIERS)
def test_full_tiles_and_grid_one_are_classic(tier, which):
    """Plain, any alpha and beta: a tile one workgroup owns whole has the
    classic launch's bits; with grid = 1 that is every tile."""
    (m, n, k), grid = split_cases(tier)[which]
    bm, bn, _ = geom(tier)
    a, b, c0 = case(m, n, k)
    want, got = c0.clone(), c0.clone()
    run(tier, "plain", a, b, want)
    run(tier, "plain", a, b, got, streamk=grid)
    torch.cuda.synchronize()
    full = [s for segs in ops.ragged_streamk_partition(tier, m, n, k, grid)[0]
            for s in segs if s[5] == "full"]
    if grid == 1:
        assert len(full) == 4
        assert torch.equal(bits(got), bits(want))
    for _, bx, by, _, _, _ in full:
        win = (slice(by * bn, (by + 1) * bn), slice(bx * bm, (bx + 1) * bm))
        assert torch.equal(bits(got[win]), bits(want[win]))


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_transposes_bit_identical(tier, mode, guarded):
    """TN, NT and TT have the bits of the NN stream-K call on
    .t().contiguous() copies with the same grid: through the fast path
    (packed operands: whole tiles and whole panels take the 16-byte forms,
    the edge tile column and the K tail the guarded ones) and with nothing
    allowing a 16-byte access (offset, odd-stride views)."""
    bm, bn, _ = geom(tier)
    m, n, k = 2 * bm, bn + 4, 3 * 64 + 8  # 4 tiles x 4 units
    grid = 5
    a, b, c0 = case(m, n, k)
    place = offset_strided if guarded else (lambda x: x)
    want = c0.clone()
    run(tier, mode, place(a), place(b), want, streamk=grid)
    at, bt = a.t().contiguous(), b.t().contiguous()
    for ta, tb in ((True, False), (False, True), (True, True)):
        got = c0.clone()
        run(tier, mode, place(at) if ta else place(a),
            place(bt) if tb else place(b), got, trans_a=ta, trans_b=tb,
            streamk=grid)
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want)), (ta, tb)
    eb.assert_within(
        want, eb.ref64(a, b, c0, ALPHA, BETA),
        eb.bound(a, b, c0, ALPHA, BETA, k) + (
            abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k, grid)
            if mode == "fused_inject" else 0),
        f"{tier} {mode} transposes")


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("grid", [3, 16])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_guard_canaries(tier, grid, mode):
    """Operands, C and the partials are views of NaN-filled parents and the
    partials are NaN themselves: an out-of-range read, or a read of a slot
    nobody wrote, makes the result non-finite; an out-of-range write changes
    a parent's bits."""
    bm, bn, _ = geom(tier)
    m, n, k = bm + 1, bn + 1, 3 * 64 + 5
    a, b, c0 = case(m, n, k)
    av, _ = bordered(a)
    bv, _ = bordered(b)
    cv, cbig = bordered(c0)
    need = ops.streamk_partials_floats(tier, grid)
    pbig = torch.full((need + 8,), NAN, device="cuda")
    assert pbig.data_ptr() % 16 == 0
    before, pbefore = cbig.clone(), pbig.clone()
    run(tier, mode, av, bv, cv, streamk=grid, partials=pbig[4:4 + need])
    torch.cuda.synchronize()
    assert torch.isfinite(cv).all()
    e = eb.bound(a, b, c0, ALPHA, BETA, k)
    if mode == "fused_inject":
        e = e + abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k, grid)
    eb.assert_within(cv, eb.ref64(a, b, c0, ALPHA, BETA), e,
                     f"{tier} {mode} canary grid {grid}")
    outside = torch.ones_like(cbig, dtype=torch.bool)
    outside[2:2 + n, 3:3 + m] = False
    assert torch.equal(cbig.view(torch.int32)[outside],
                       before.view(torch.int32)[outside])
    for part in (slice(0, 4), slice(4 + need, None)):
        assert torch.equal(bits(pbig[part]), bits(pbefore[part]))


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_beta_zero_never_reads_c(tier, mode):
    """grid 3 holds fully-owned tiles (direct epilogue) and split ones
    (fixup pass)."""
    bm, bn, _ = geom(tier)
    m, n, k = bm + 1, bn + 1, 3 * 64 + 5
    a, b, _ = case(m, n, k)
    kinds = {s[5] for segs in
             ops.ragged_streamk_partition(tier, m, n, k, 3)[0] for s in segs}
    assert kinds == {"full", "head", "tail"}
    c = torch.full((n, m), NAN, device="cuda")
    run(tier, mode, a, b, c, ALPHA, 0.0, streamk=3)
    torch.cuda.synchronize()
    assert torch.isfinite(c).all()
    eb.assert_within(c, eb.ref64(a, b, None, ALPHA, 0.0),
                     eb.bound(a, b, None, ALPHA, 0.0, k),
                     f"{tier} {mode} beta 0")


@pytest.mark.parametrize("vw", [20, 2])
@pytest.mark.parametrize("grid", [3, 5])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_injection_and_report(tier, grid, vw):
    """Segments of up to four units; with verify_windows = 20 every unit is
    a group, with 2 a group is two units and a segment ends in a short one.
    Events are the predictor's, all corrected, and the report changes no
    bit of C."""
    bm, bn, _ = geom(tier)
    m, n, k = bm + 1, bn + 1, 3 * 64 + 5
    a, b, c0 = case(m, n, k)
    want = predict_injected_events(tier, m, n, k, vw, ragged=True,
                                   streamk_grid=grid)
    assert len(want) > len(ops.ragged_streamk_partition(tier, m, n, k,
                                                        grid)[0])
    rep = FaultReport(capacity=256)
    c, c_norep = c0.clone(), c0.clone()
    ops.ft_sgemm_ragged(tier, a, b, c, ALPHA, BETA, inject=True,
                        verify_windows=vw, report=rep, streamk=grid)
    ops.ft_sgemm_ragged(tier, a, b, c_norep, ALPHA, BETA, inject=True,
                        verify_windows=vw, streamk=grid)
    r = rep.read()
    key = lambda e: (e.i, e.j, e.k_begin, e.k_end, e.status)  # noqa: E731
    assert sorted(map(key, r.events)) == sorted(map(key, want))
    assert r.corrected == len(want) and r.tripped == len(want)
    assert r.uncorrected == 0 and r.unlocated == 0 and r.dropped == 0
    assert torch.equal(bits(c), bits(c_norep))
    eb.assert_within(
        c, eb.ref64(a, b, c0, ALPHA, BETA),
        eb.bound(a, b, c0, ALPHA, BETA, k) +
        abs(ALPHA) * FAULT_TOL * site_counts(tier, m, n, k, grid, vw),
        f"{tier} inject grid {grid} vw {vw}")


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("tier", SK_TIERS)
def test_no_false_trips(tier, which):
    (m, n, k), grid = split_cases(tier)[which]
    a, b, c0 = case(m, n, k)
    rep = FaultReport(capacity=16)
    c = c0.clone()
    ops.ft_sgemm_ragged(tier, a, b, c, ALPHA, BETA, inject=False, tau=100.0,
                        report=rep, streamk=grid)
    r = rep.read()
    assert (r.tripped, r.n_events, r.unlocated) == (0, 0, 0)


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_deterministic_and_capturable(tier, mode):
    """Two eager runs have the same bits, and so has one launch captured in
    a graph (caller-owned partials, a single linear chain) and replayed."""
    bm, bn, _ = geom(tier)
    m, n, k = bm + 1, bn + 1, 3 * 64 + 5
    grid = 5
    a, b, c0 = case(m, n, k)
    partials = torch.empty(ops.streamk_partials_floats(tier, grid),
                           device="cuda")
    eager = []
    for _ in range(2):
        c = c0.clone()
        run(tier, mode, a, b, c, streamk=grid, partials=partials)
        eager.append(c)
    torch.cuda.synchronize()
    assert torch.equal(bits(eager[0]), bits(eager[1]))
    c = c0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(tier, mode, a, b, c, streamk=grid, partials=partials)
    c.copy_(c0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(eager[0]))


def test_auto_grid_is_the_device_grid():
    """"auto" asks the device: CUs x resident workgroups, clamped to the
    unit count, the same with and without a report; the result is within
    the bound."""
    tier = "huge"
    m, n, k = 300, 200, 64 * 40 + 3
    a, b, c0 = case(m, n, k)
    ti = ops.tier_index(tier)
    g = ops._C.ragged_streamk_grid(ti, True, False, m, n, k)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    units = 2 * 2 * 41
    assert g == min(units, g) and g >= 1
    assert g == units or g % cus == 0
    assert ops._C.ragged_streamk_grid(ops.tier_index("medium"), True, False,
                                      m, n, k) == 0
    c = c0.clone()
    run(tier, "fused", a, b, c, streamk="auto")
    c_rep = c0.clone()
    run(tier, "fused", a, b, c_rep, streamk="auto", report=FaultReport(16))
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(c_rep))
    eb.assert_within(c, eb.ref64(a, b, c0, ALPHA, BETA),
                     eb.bound(a, b, c0, ALPHA, BETA, k), "huge auto")


def test_rules():
    m, n, k = 65, 65, 197
    a, b, c0 = case(m, n, k)
    c = c0.clone()
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.sgemm_ragged("medium", a, b, c, streamk=4)
    with pytest.raises(TypeError):  # the batched entries have no stream-K
        ops.sgemm_ragged_batched("large", a[None], b[None], c[None],
                                 streamk=4)
    with pytest.raises(ValueError, match="2-D"):
        ops.sgemm_ragged("large", a[None], b[None], c[None], streamk=4)
    need = ops.streamk_partials_floats("large", 4)
    buf = torch.empty(need + 4, device="cuda")
    with pytest.raises(ValueError, match="16-byte"):
        ops.sgemm_ragged("large", a, b, c, streamk=4, partials=buf[1:1 + need])
    with pytest.raises(ValueError, match="needs"):
        ops.sgemm_ragged("large", a, b, c, streamk=4, partials=buf[:need - 1])
    with pytest.raises(ValueError, match="partials go with"):
        ops.sgemm_ragged("large", a, b, c, partials=buf)
    # the binding holds the same line for a caller that skips the mirror
    ti = ops.tier_index("large")
    args = (ti, False, False, a, b, c, 1.0, 0.0, 0.0, 0.0, 20, None, None)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops._C.sgemm_ragged(*args, sk_grid=4, partials=buf[1:1 + need])
    with pytest.raises(RuntimeError, match="needs"):
        ops._C.sgemm_ragged(*args, sk_grid=4, partials=buf[:need - 4])
    with pytest.raises(RuntimeError, match="no stream-K twin"):
        ops._C.sgemm_ragged(ops.tier_index("medium"), *args[1:], sk_grid=4,
                            partials=buf)
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(c0))  # nothing was launched


@pytest.mark.parametrize("tier", ["large", None])
def test_ft_linear_streamk(monkeypatch, tier):
    """With the gate forced open every product of ft_linear takes the
    stream-K launch, on the caller's tier or, with none given, on huge, the
    first tier the gate is asked about; y, grad_x and grad_weight stay
    within the bound of the fp64 products."""
    monkeypatch.setattr(ops, "ragged_streamk_gate",
                        lambda tier, m, n, k, fused: True)
    seen = []
    real = ops.ft_sgemm_ragged

    def spy(*args, **kw):
        seen.append((args[0], kw.get("streamk")))
        return real(*args, **kw)

    monkeypatch.setattr(ops, "ft_sgemm_ragged", spy)
    tokens, fin, fout = 200, 70, 66
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.rand((tokens, fin), generator=g) * 1.8 - 0.9).cuda()
    w = (torch.rand((fout, fin), generator=g) * 1.8 - 0.9).cuda()
    gy = (torch.rand((tokens, fout), generator=g) * 1.8 - 0.9).cuda()
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = ops.ft_linear(x, w, tier=tier, streamk=True)
    y.backward(gy)
    torch.cuda.synchronize()
    assert seen == [(tier or "huge", "auto")] * 3
    xd, wd = x.detach(), w.detach()
    # in the kernels' terms c (N, M) = b (K, N)^T a (K, M)
    for got, a, b, kk, what in (
            (y.detach(), wd.t(), xd.t(), fin, "y"),
            (x.grad, wd, gy.t(), fout, "grad_x"),
            (w.grad, xd, gy, tokens, "grad_weight")):
        eb.assert_within(got, eb.ref64(a, b, None, 1.0, 0.0),
                         eb.bound(a, b, None, 1.0, 0.0, kk),
                         f"ft_linear streamk {what}")
