"""GPU tests of the grouped stream-K launch (ops.GroupedPlan, sgemm_grouped
and ft_sgemm_grouped with streamk=, ft_grouped_linear with streamk=).

One group per tier with tile (bm, bn): an entry one row and one column past
a tile with a short last unit, a tiny entry, an entry without tiles, a K == 0
entry of one tile, a six-tile entry and a one-element entry, 37 units in all.
tests/test_grouped_streamk_cpu.py asserts that with GRIDS the group holds a
fully-owned tile, a tile split over two workgroups, one split over three or
more with a workgroup wholly inside it, a workgroup with head + full + tail,
a workgroup that crosses an entry boundary, a K == 0 tile at the start and in
the middle of a workgroup's range, and an empty entry between live ones.
Numerics are checked against the fp64 reference within the bound of
utils/errbound.py, which holds for any summation order and so needs no
widening for the slot sum; a corrected fault site gets the project's
|alpha| * 1e-2 on top.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TILING
from ft_sgemm_amd.ops.fault_report import (BatchedFaultReport,
                                           predict_injected_events_grouped)
from ft_sgemm_amd.utils import errbound as eb

SK_TIERS = ("large", "huge")
GRIDS = (1, 3, 5, 7, 16, 40)  # 37 units: 40 is clamped
ALPHA, BETA = 1.5, -0.5
FAULT_TOL = 1e-2  # per corrected fault, tests/test_gpu_threshold.py
NAN = float("nan")


def group(tier):
    bm, bn = TILING[tier]["bm"], TILING[tier]["bn"]
    return [(bm + 1, bn + 1, 3 * 64 + 5), (3, 5, 7), (0, 5, 9), (bm, bn, 0),
            (2 * bm + 1, bn + 1, 2 * 64 + 5), (1, 1, 1)]


_ops = {}


def operands(tier):
    """Seeded packed (a_list, b_list, c0_list) of the tier's group, made once
    and never written."""
    if tier not in _ops:
        al, bl, cl = [], [], []
        for e, (m, n, k) in enumerate(group(tier)):
            g = torch.Generator(device="cpu").manual_seed(
                97 * e + 7 * m + 3 * n + k)
            al.append((torch.rand((k, m), generator=g) * 1.8 - 0.9).cuda())
            bl.append((torch.rand((k, n), generator=g) * 1.8 - 0.9).cuda())
            cl.append(torch.randn((n, m), generator=g).cuda())
        _ops[tier] = (al, bl, cl)
    return _ops[tier]


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
    16-byte access.  (The single-launch test's helper, for any width.)"""
    r, c = x.shape
    if x.numel() == 0:
        return x
    ld = c + 1 if (c + 1) % 4 else c + 2
    flat = torch.zeros(r * ld + 1, device=x.device)
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided((r, c), (ld, 1), 1)
    view.copy_(x)
    return view


def run(tier, mode, al, bl, cl, alpha=ALPHA, beta=BETA, **kw):
    if mode == "plain":
        return ops.sgemm_grouped(tier, al, bl, cl, alpha, beta, **kw)
    return ops.ft_sgemm_grouped(tier, al, bl, cl, alpha, beta,
                                inject=(mode == "fused_inject"), **kw)


def single(tier, mode, a, b, c, alpha, beta):
    if mode == "plain":
        return ops.sgemm_ragged(tier, a, b, c, alpha, beta)
    return ops.ft_sgemm_ragged(tier, a, b, c, alpha, beta, inject=False)


def bits(x):
    return x.contiguous().view(torch.int32)


def clones(cl):
    return [c.clone() for c in cl]


def window(tier, shape, bx, by):
    bm, bn = TILING[tier]["bm"], TILING[tier]["bn"]
    m, n, _ = shape
    return (slice(by * bn, min(n, (by + 1) * bn)),
            slice(bx * bm, min(m, (bx + 1) * bm)))


def site_counts(tier, grid, vw=20):
    """Per entry (n, m) fp64: predicted corrected injections per element."""
    out = []
    for (m, n, _), ev in zip(group(tier), predict_injected_events_grouped(
            tier, group(tier), vw, grid)):
        v = torch.zeros((n, m), dtype=torch.float64)
        for e in ev:
            if e.i < m and e.j < n:
                v[e.j, e.i] += 1
        out.append(v.cuda())
    return out


def check_within(tier, al, bl, c0l, got, alpha, beta, what, extra=None):
    for e, (m, n, k) in enumerate(group(tier)):
        if m == 0 or n == 0:
            continue
        bound = eb.bound(al[e], bl[e], c0l[e], alpha, beta, k)
        if extra is not None:
            bound = bound + abs(alpha) * FAULT_TOL * extra[e]
        eb.assert_within(got[e], eb.ref64(al[e], bl[e], c0l[e], alpha, beta),
                         bound, f"{what} entry {e}")


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("tier", SK_TIERS)
def test_numerics(tier, grid, mode):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    al, bl, c0l = operands(tier)
    got = clones(c0l)
    run(tier, mode, al, bl, got, streamk=grid)
    torch.cuda.synchronize()
    check_within(tier, al, bl, c0l, got, ALPHA, BETA,
                 f"{tier} {mode} grid {grid}")


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("tier", SK_TIERS)
def test_fully_owned_tiles_are_classic(tier, grid, mode):
    """Any alpha and beta: a tile one workgroup owns whole has the classic
    grouped launch's bits; with grid = 1 that is every tile."""
    al, bl, c0l = operands(tier)
    want, got = clones(c0l), clones(c0l)
    run(tier, mode, al, bl, want)
    run(tier, mode, al, bl, got, streamk=grid)
    torch.cuda.synchronize()
    shapes = group(tier)
    full = [s for segs in ops.grouped_streamk_partition(tier, shapes, grid)[0]
            for s in segs if s[6] == "full"]
    assert full
    if grid == 1:
        assert len(full) == 13
    for e, _, bx, by, _, _, _ in full:
        win = window(tier, shapes[e], bx, by)
        assert torch.equal(bits(got[e][win]), bits(want[e][win])), (e, bx, by)


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("grid", GRIDS[1:])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_split_tiles_bit_composition(tier, grid, mode):
    """alpha = 1, beta = 0: every split tile is, bit for bit, the
    left-to-right fp32 sum of the classic single ragged launch's results on
    the K slices of the tile's segments, in workgroup order."""
    al, bl, c0l = operands(tier)
    shapes = group(tier)
    got = [torch.empty_like(c) for c in c0l]
    run(tier, mode, al, bl, got, 1.0, 0.0, streamk=grid)
    slices = {}

    def classic(e, w_lo, w_hi):
        if (e, w_lo, w_hi) not in slices:
            lo, hi = 64 * w_lo, min(shapes[e][2], 64 * w_hi)
            out = torch.empty_like(c0l[e])
            single(tier, mode, al[e][lo:hi], bl[e][lo:hi], out, 1.0, 0.0)
            slices[(e, w_lo, w_hi)] = out
        return slices[(e, w_lo, w_hi)]

    per_tile = {}
    for segs in ops.grouped_streamk_partition(tier, shapes, grid)[0]:
        for e, _, bx, by, w_lo, w_hi, kind in segs:
            if kind != "full":
                per_tile.setdefault((e, bx, by), []).append((w_lo, w_hi))
    assert per_tile
    for (e, bx, by), segs in per_tile.items():
        win = window(tier, shapes[e], bx, by)
        s = classic(e, *segs[0])[win].clone()
        for seg in segs[1:]:
            s = s + classic(e, *seg)[win]
        assert torch.equal(bits(got[e][win]), bits(s)), (e, bx, by)


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("grid", [5, 16])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_k_zero_and_empty_entries(tier, grid, mode):
    """The K == 0 entry (index 3) becomes beta * c0 exactly, exact zeros
    with a NaN c going in for beta == 0; its report slot and the empty
    entry's (index 2) are untouched."""
    al, bl, c0l = operands(tier)
    rep = None
    if mode != "plain":
        rep = BatchedFaultReport(len(c0l), capacity=64)
        rep.counters[2:4] = 77
        rep.events[2:4] = -7
    kw = {} if rep is None else {"report": rep}
    got = clones(c0l)
    run(tier, mode, al, bl, got, ALPHA, BETA, streamk=grid, **kw)
    assert torch.equal(bits(got[3]), bits(c0l[3] * BETA))
    got = clones(c0l)
    got[3].fill_(NAN)
    run(tier, mode, al, bl, got, ALPHA, 0.0, streamk=grid, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(got[3]), torch.zeros_like(bits(got[3])))
    assert all(torch.isfinite(c).all() for c in got)
    if rep is not None:
        assert (rep.counters[2:4] == 77).all() and (rep.events[2:4] == -7).all()
        assert int(rep.counters[0, 0]) > 0


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_footprint(tier, mode, guarded):
    """Operands and C are views of NaN-filled parents (or offset, odd-stride
    views) and the partials are NaN with canaries on both sides: an
    out-of-range read, or a read of a slot nobody wrote, makes the result
    non-finite; an out-of-range write changes a parent's bits.  The fused
    plan's workspace is the queried size, filled with NaN before the run:
    the encode must rewrite all of it that is read."""
    grid = 7
    al, bl, c0l = operands(tier)
    shapes = group(tier)
    if guarded:
        av, bv = [offset_strided(x) for x in al], \
            [offset_strided(x) for x in bl]
    else:
        av = [bordered(x)[0] for x in al]
        bv = [bordered(x)[0] for x in bl]
    cv, cbig = zip(*[bordered(c) for c in c0l])
    need = ops.streamk_partials_floats(tier, grid)
    pbig = torch.full((need + 8,), NAN, device="cuda")
    assert pbig.data_ptr() % 16 == 0
    before, pbefore = [c.clone() for c in cbig], pbig.clone()
    fused = mode != "plain"
    plan = ops.GroupedPlan(tier, av, bv, list(cv), fused=fused, streamk=grid,
                           partials=pbig[4:4 + need])
    assert plan.streamk_grid == grid
    wm = TILING[tier]["wm"]
    assert plan.workspace.numel() == (sum(
        2 * -(-m // wm) * (-(-k // 64) * 64)
        for m, n, k in shapes if min(m, n, k) > 0) if fused else 0)
    plan.workspace.fill_(NAN)
    plan.run(ALPHA, BETA, inject=fused)
    torch.cuda.synchronize()
    assert all(torch.isfinite(c).all() for c in cv)
    check_within(tier, al, bl, c0l, cv, ALPHA, BETA,
                 f"{tier} {mode} footprint",
                 site_counts(tier, grid) if fused else None)
    for (m, n, _), big, was in zip(shapes, cbig, before):
        outside = torch.ones_like(big, dtype=torch.bool)
        outside[2:2 + n, 3:3 + m] = False
        assert torch.equal(big.view(torch.int32)[outside],
                           was.view(torch.int32)[outside])
    for part in (slice(0, 4), slice(4 + need, None)):
        assert torch.equal(bits(pbig[part]), bits(pbefore[part]))


@pytest.mark.parametrize("mode", ["plain", "fused_inject"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_transposes_bit_identical(tier, mode):
    """TN, NT and TT have the bits of the NN stream-K call on
    .t().contiguous() copies with the same grid."""
    grid = 5
    al, bl, c0l = operands(tier)
    want = clones(c0l)
    run(tier, mode, al, bl, want, streamk=grid)
    at = [x.t().contiguous() for x in al]
    bt = [x.t().contiguous() for x in bl]
    for ta, tb in ((True, False), (False, True), (True, True)):
        got = clones(c0l)
        run(tier, mode, at if ta else al, bt if tb else bl, got, trans_a=ta,
            trans_b=tb, streamk=grid)
        torch.cuda.synchronize()
        for e in range(len(got)):
            assert torch.equal(bits(got[e]), bits(want[e])), (ta, tb, e)
    check_within(tier, al, bl, c0l, want, ALPHA, BETA,
                 f"{tier} {mode} transposes",
                 site_counts(tier, grid) if mode != "plain" else None)


@pytest.mark.parametrize("vw", [20, 2])
@pytest.mark.parametrize("grid", [3, 7])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_injection_and_report(tier, grid, vw):
    """Per entry the events are the predictor's, all corrected; counts and
    bits are the same with and without a report attached."""
    al, bl, c0l = operands(tier)
    shapes = group(tier)
    want = predict_injected_events_grouped(tier, shapes, vw, grid)
    rep = BatchedFaultReport(len(shapes), capacity=256)
    c, c_norep = clones(c0l), clones(c0l)
    ops.ft_sgemm_grouped(tier, al, bl, c, ALPHA, BETA, inject=True,
                         verify_windows=vw, report=rep, streamk=grid)
    ops.ft_sgemm_grouped(tier, al, bl, c_norep, ALPHA, BETA, inject=True,
                         verify_windows=vw, streamk=grid)
    key = lambda e: (e.i, e.j, e.k_begin, e.k_end, e.status)  # noqa: E731
    for e, r in enumerate(rep.read()):
        assert sorted(map(key, r.events)) == sorted(map(key, want[e])), e
        assert r.corrected == len(want[e]) and r.tripped == len(want[e])
        assert r.uncorrected == 0 and r.unlocated == 0 and r.dropped == 0
        assert torch.equal(bits(c[e]), bits(c_norep[e]))
    assert sum(map(len, want)) > 0
    check_within(tier, al, bl, c0l, c, ALPHA, BETA,
                 f"{tier} inject grid {grid} vw {vw}",
                 site_counts(tier, grid, vw))


@pytest.mark.parametrize("mode", ["plain", "fused"])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_deterministic_and_capturable(tier, mode):
    """Two runs of one plan have the same bits, and so has plan.run captured
    in a graph (a single linear chain) and replayed."""
    al, bl, c0l = operands(tier)
    c = clones(c0l)
    plan = ops.GroupedPlan(tier, al, bl, c, fused=(mode == "fused"),
                           streamk=5)
    assert plan.partials.numel() == ops.streamk_partials_floats(tier, 5)
    eager = []
    for _ in range(2):
        for x, x0 in zip(c, c0l):
            x.copy_(x0)
        plan.run(ALPHA, BETA)
        eager.append(clones(c))
    torch.cuda.synchronize()
    for x, y in zip(*eager):
        assert torch.equal(bits(x), bits(y))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run(ALPHA, BETA)
    for x, x0 in zip(c, c0l):
        x.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(c, eager[0]):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("tier", SK_TIERS)
def test_auto_grid_and_streamk_zero(tier):
    """"auto" asks the device: a positive grid of at most the unit count,
    the same with and without a report; streamk=0 is the classic launch."""
    al, bl, c0l = operands(tier)
    c = clones(c0l)
    plan = ops.GroupedPlan(tier, al, bl, c, fused=True, streamk="auto")
    assert 1 <= plan.streamk_grid <= 37
    plan.run(ALPHA, BETA)
    c_rep = clones(c0l)
    ops.ft_sgemm_grouped(tier, al, bl, c_rep, ALPHA, BETA, inject=False,
                         streamk="auto",
                         report=BatchedFaultReport(len(c0l), 16))
    torch.cuda.synchronize()
    for x, y in zip(c, c_rep):
        assert torch.equal(bits(x), bits(y))
    check_within(tier, al, bl, c0l, c, ALPHA, BETA, f"{tier} auto")
    classic, zero = clones(c0l), clones(c0l)
    ops.ft_sgemm_grouped(tier, al, bl, classic, ALPHA, BETA, inject=False)
    p0 = ops.GroupedPlan(tier, al, bl, zero, fused=True, streamk=0)
    assert p0.streamk_grid == 0 and p0.partials is None
    p0.run(ALPHA, BETA)
    torch.cuda.synchronize()
    for x, y in zip(zero, classic):
        assert torch.equal(bits(x), bits(y))


def test_rules():
    al, bl, c0l = operands("large")
    c = clones(c0l)
    need = ops.streamk_partials_floats("large", 4)
    buf = torch.empty(need + 4, device="cuda")
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.sgemm_grouped("medium", al, bl, c, streamk=4)
    with pytest.raises(ValueError, match="16-byte"):
        ops.sgemm_grouped("large", al, bl, c, streamk=4,
                          partials=buf[1:1 + need])
    with pytest.raises(ValueError, match="needs"):
        ops.sgemm_grouped("large", al, bl, c, streamk=4,
                          partials=buf[:need - 1])
    # the binding holds the same line for a caller that skips the mirror
    ti = ops.tier_index("large")
    args = (False, al, bl, c, False, False, 20)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops._C.GroupedPlan(ti, *args, sk_grid=4, partials=buf[1:1 + need])
    with pytest.raises(RuntimeError, match="needs"):
        ops._C.GroupedPlan(ti, *args, sk_grid=4, partials=buf[:need - 4])
    with pytest.raises(RuntimeError, match="no stream-K twin"):
        ops._C.GroupedPlan(ops.tier_index("medium"), *args, sk_grid=4)
    with pytest.raises(RuntimeError, match="partials go with"):
        ops._C.GroupedPlan(ti, *args, sk_grid=0, partials=buf)
    # a group without units plans the classic launch, which launches nothing
    e = ops.GroupedPlan("large", al[2:3], bl[2:3], c[2:3], streamk=4)
    assert e.streamk_grid == 0
    e.run()
    torch.cuda.synchronize()
    for x, y in zip(c, c0l):
        assert torch.equal(bits(x), bits(y))  # nothing was launched


def test_ft_grouped_linear_streamk():
    """counts [70, 0, 5, 130], in 72, out 40, with bias, on tier large:
    "always" runs all three products as grouped stream-K launches and stays
    within the bound of the fp64 torch reference, the token-less expert's
    grad_weight exactly zero; False gives today's bits and so does True,
    since the gate is False at this small shape."""
    counts, fin, fout = [70, 0, 5, 130], 72, 40
    tokens, experts = sum(counts), len(counts)
    g = torch.Generator(device="cpu").manual_seed(9)
    x0 = (torch.rand((tokens, fin), generator=g) * 1.8 - 0.9).cuda()
    w0 = (torch.rand((experts, fout, fin), generator=g) * 1.8 - 0.9).cuda()
    b0 = (torch.rand((experts, fout), generator=g) * 1.8 - 0.9).cuda()
    gy = (torch.rand((tokens, fout), generator=g) * 1.8 - 0.9).cuda()

    seen = []
    real = ops.ft_sgemm_grouped

    def spy(*args, **kw):
        seen.append(kw.get("streamk"))
        return real(*args, **kw)

    def go(streamk):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        y = ops.ft_grouped_linear(x, w, counts, b, tier="large",
                                  streamk=streamk)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), x.grad, w.grad, b.grad

    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "ft_sgemm_grouped", spy)
    try:
        always = go("always")
        assert seen == ["auto"] * 3
        del seen[:]
        base, gated = go(False), go(True)
        assert seen == [0] * 6
    finally:
        mp.undo()
    assert ops.grouped_streamk_gate(
        "large", [(fin, fout, n) for n in counts], True) is False
    # y, grad_x, grad_weight: the three products.  grad_bias is torch's
    # index_add_, whose float atomics fix no order: it is bounded below, not
    # compared bit for bit.
    for what, u, v in zip(("y", "grad_x", "grad_weight"), base, gated):
        assert torch.equal(bits(u), bits(v)), what
    y, gx, gw, gb = always
    assert torch.equal(bits(gw[1]), torch.zeros_like(bits(gw[1])))
    row = 0
    for e, n in enumerate(counts):
        rows = slice(row, row + n)
        row += n
        xe, ge, we = x0[rows], gy[rows], w0[e]
        bias = b0[e].expand(n, fout)
        # in the kernels' terms c (N, M) = b (K, N)^T a (K, M)
        if n:
            eb.assert_within(y[rows], eb.ref64(we.t(), xe.t(), bias, 1.0, 1.0),
                             eb.bound(we.t(), xe.t(), bias, 1.0, 1.0, fin),
                             f"y expert {e}")
            eb.assert_within(gx[rows], eb.ref64(we, ge.t(), None, 1.0, 0.0),
                             eb.bound(we, ge.t(), None, 1.0, 0.0, fout),
                             f"grad_x expert {e}")
        eb.assert_within(gw[e], eb.ref64(xe, ge, None, 1.0, 0.0),
                         eb.bound(xe, ge, None, 1.0, 0.0, n),
                         f"grad_weight expert {e}")
        # grad_bias: a torch fp32 segment sum of n terms, any order
        ref = ge.double().sum(0)
        lim = (n + 8) * eb.EPS * ge.double().abs().sum(0)
        assert ((gb[e].double() - ref).abs() <= lim).all()
