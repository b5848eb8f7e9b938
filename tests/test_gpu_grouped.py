"""GPU tests of the grouped ragged launch (ops.sgemm_grouped /
ops.ft_sgemm_grouped / ops.GroupedPlan): entry e of one launch must have the
bits, and report the fault events, of the single ragged launch
(ops.sgemm_ragged / ops.ft_sgemm_ragged) on its own operands.  Shapes are a few
tiles of each tier; every comparison is bit for bit, so there is no
tolerance."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import kernel_table as kt
from ft_sgemm_amd import ops
from ft_sgemm_amd.ops.fault_report import FaultCounts, FaultReport

TRANS = [(False, False), (True, False), (False, True), (True, True)]
ALPHA, BETA = 1.5, -0.5


def rand(g, *shape):
    return (torch.rand(shape, generator=g) * 1.8 - 0.9).cuda()


def make_entry(g, m, n, k, ta, tb):
    """(a, b, c) of one entry; c holds values for beta to scale."""
    return (rand(g, *((m, k) if ta else (k, m))),
            rand(g, *((n, k) if tb else (k, n))), rand(g, n, m))


def make_group(shapes, ta, tb, seed=7):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return tuple(map(list, zip(*(make_entry(g, *s, ta, tb) for s in shapes))))


def single(tier, a, b, c, alpha, beta, ta, tb, fused=False, **kw):
    """The single ragged launch on a copy of c; returns (c, FaultCounts)."""
    out = c.clone()
    if not fused:
        ops.sgemm_ragged(tier, a, b, out, alpha, beta, trans_a=ta, trans_b=tb)
        return out, None
    rep = FaultReport() if kw.get("inject") else None
    ops.ft_sgemm_ragged(tier, a, b, out, alpha, beta, report=rep, trans_a=ta,
                        trans_b=tb, **kw)
    return out, rep.read() if rep is not None else None


def tier_shapes(tier):
    """The issue's group for one tier, in its order: the big entry is not
    first, one entry has no columns, the last has several verify windows."""
    t = kt.TILING[tier]
    bm, bn, bk = t["bm"], t["bn"], t["bk"]
    return [(1, 1, 1), (bm + 1, bn - 1, bk + 1), (2 * bm, 2 * bn, 64),
            (bm, 0, bk), (7, 9, 5 * bk + 3)]


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("tier", kt.TIERS)
def test_plain_entries_have_the_single_launch_bits(tier, ta, tb):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    shapes = tier_shapes(tier)
    a, b, c = make_group(shapes, ta, tb)
    want = [single(tier, x, y, z, ALPHA, BETA, ta, tb)[0] if s[1] else z
            for s, x, y, z in zip(shapes, a, b, c)]
    got = ops.sgemm_grouped(tier, a, b, c, ALPHA, BETA, trans_a=ta,
                            trans_b=tb)
    torch.cuda.synchronize()
    for e, (w, x) in enumerate(zip(want, got)):
        assert x is c[e]
        assert torch.equal(w, x), f"entry {e} {shapes[e]}"


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("tier", kt.TIERS)
def test_fused_entries_have_the_single_launch_bits_and_events(tier, ta, tb):
    shapes = tier_shapes(tier)
    a, b, c = make_group(shapes, ta, tb)
    want = [single(tier, x, y, z, ALPHA, BETA, ta, tb, fused=True,
                   inject=True) if s[1] else (z, FaultCounts())
            for s, x, y, z in zip(shapes, a, b, c)]
    rep = ops.BatchedFaultReport(len(shapes))
    ops.ft_sgemm_grouped(tier, a, b, c, ALPHA, BETA, inject=True, report=rep,
                         trans_a=ta, trans_b=tb)
    got = rep.read()
    assert sum(r.corrected for r in got) > 0
    for e, ((w, counts), x) in enumerate(zip(want, c)):
        assert torch.equal(w, x), f"entry {e} {shapes[e]}"
        assert got[e] == counts, f"entry {e} {shapes[e]}"
    # several verify windows in the last entry: one event per window
    assert len({ev.k_begin for ev in got[-1].events}) > 1


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tier,ta,tb", [("medium", False, False),
                                        ("huge", True, True),
                                        ("large", False, True)])
def test_k_zero_entry_is_beta_c(tier, ta, tb, fused):
    t = kt.TILING[tier]
    shapes = [(t["bm"] + 3, t["bn"] + 2, 0), (t["bm"] + 1, 5, 37)]
    call = ops.ft_sgemm_grouped if fused else ops.sgemm_grouped
    for beta in (BETA, 0.0):
        a, b, c = make_group(shapes, ta, tb, seed=11)
        c0 = c[0].clone()
        want1 = single(tier, a[1], b[1], c[1], ALPHA, beta, ta, tb,
                       fused=fused, inject=True)[0]
        if beta == 0.0:
            c[0].fill_(float("nan"))  # must not be read
        rep = ops.BatchedFaultReport(2) if fused else None
        kw = dict(inject=True, report=rep) if fused else {}
        call(tier, a, b, c, ALPHA, beta, trans_a=ta, trans_b=tb, **kw)
        torch.cuda.synchronize()
        if beta == 0.0:
            assert torch.equal(c[0], torch.zeros_like(c0))
        else:
            assert torch.equal(c[0], beta * c0)
        assert torch.equal(c[1], want1)
        if fused:  # an entry without panels injects and reports nothing
            r = rep.read()
            assert r[0] == FaultCounts() and r[1].corrected > 0


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tier,ta,tb", [("huge", False, False),
                                        ("huge", True, True),
                                        ("small", True, False)])
def test_misaligned_entries_sit_next_to_aligned_ones(tier, ta, tb, fused):
    """Every entry is a 16-byte-path candidate by its leading dimensions; in
    entries 1, 2 and 3 one of A, B, C starts one float past a 16-byte
    boundary, so the kernel must settle the fast bits per entry."""
    t = kt.TILING[tier]
    m, n, k = 2 * t["bm"], 2 * t["bn"], 64
    g = torch.Generator(device="cpu").manual_seed(23)

    def shifted(shape, off):
        flat = rand(g, shape[0] * shape[1] + 4)
        assert flat.data_ptr() % 16 == 0
        return flat[off:off + shape[0] * shape[1]].view(shape)

    a, b, c = [], [], []
    for e in range(4):
        a.append(shifted((m, k) if ta else (k, m), int(e == 1)))
        b.append(shifted((n, k) if tb else (k, n), int(e == 2)))
        c.append(shifted((n, m), int(e == 3)))
    assert a[1].data_ptr() % 16 == 4 and c[3].data_ptr() % 16 == 4
    want = [single(tier, x, y, z, ALPHA, BETA, ta, tb, fused=fused,
                   inject=False)[0] for x, y, z in zip(a, b, c)]
    if fused:
        ops.ft_sgemm_grouped(tier, a, b, c, ALPHA, BETA, inject=False,
                             trans_a=ta, trans_b=tb)
    else:
        ops.sgemm_grouped(tier, a, b, c, ALPHA, BETA, trans_a=ta, trans_b=tb)
    torch.cuda.synchronize()
    for e in range(4):
        assert torch.equal(want[e], c[e]), f"entry {e}"


def test_entries_are_isolated():
    """All C entries inside one buffer with NaN guard bands between them: the
    bands stay untouched bit for bit, and a NaN in one entry's A poisons
    that entry's C only."""
    tier = "large"
    shapes = [(65, 63, 17), (3, 5, 40), (64, 64, 64), (10, 0, 8), (33, 2, 9)]
    a, b, _ = make_group(shapes, False, False, seed=31)
    a[1][3, 1] = float("nan")
    band = 13
    total = sum(m * n + band for m, n, _ in shapes) + band
    buf = torch.full((total,), float("nan"), device="cuda")
    before = buf.view(torch.int32).clone()
    c, written, off = [], torch.zeros(total, dtype=torch.bool), band
    for m, n, _ in shapes:
        c.append(buf[off:off + m * n].view(n, m))
        written[off:off + m * n] = True
        off += m * n + band
    want = [single(tier, x, y, torch.zeros_like(z), 1.0, 0.0, False, False)[0]
            if s[1] else z.clone() for s, x, y, z in zip(shapes, a, b, c)]
    ops.sgemm_grouped(tier, a, b, c, 1.0, 0.0)
    torch.cuda.synchronize()
    guard = ~written.cuda()
    assert torch.equal(buf.view(torch.int32)[guard], before[guard])
    for e, (w, x) in enumerate(zip(want, c)):
        assert torch.equal(w.view(torch.int32), x.view(torch.int32)), e
        if shapes[e][1]:
            assert bool(torch.isnan(x).any()) == (e == 1), e


def test_workspace_is_fully_rewritten():
    """A workspace full of NaN before run(): the encode must write every
    element that is read, the zero fill of [K_e, sstr_e) included."""
    tier = "tall"
    shapes = [(130, 33, 70), (5, 7, 1), (64, 40, 129), (9, 9, 63)]
    for ta in (False, True):
        a, b, c = make_group(shapes, ta, False, seed=41)
        want = [single(tier, x, y, z, ALPHA, BETA, ta, False, fused=True,
                       inject=False)[0] for x, y, z in zip(a, b, c)]
        plan = ops.GroupedPlan(tier, a, b, c, fused=True, trans_a=ta)
        wm = kt.TILING[tier]["wm"]
        assert plan.workspace.numel() == sum(
            2 * -(-m // wm) * (-(-k // 64) * 64) for m, _, k in shapes)
        plan.workspace.fill_(float("nan"))
        plan.run(ALPHA, BETA)
        torch.cuda.synchronize()
        for e in range(len(shapes)):
            assert torch.equal(want[e], c[e]), f"trans_a={ta} entry {e}"


def test_more_entries_than_a_grid_dimension():
    """70000 one-element entries and one two-tile entry in the middle: no
    limit of 65535 entries, and the lookup works on a long table."""
    tier, n1 = "small", 70000
    g = torch.Generator(device="cpu").manual_seed(53)
    a_all, b_all = rand(g, n1), rand(g, n1)
    c_all = torch.full((n1,), float("nan"), device="cuda")
    a = list(a_all.view(n1, 1, 1).unbind(0))
    b = list(b_all.view(n1, 1, 1).unbind(0))
    c = list(c_all.view(n1, 1, 1).unbind(0))
    bm = kt.TILING[tier]["bm"]
    big = make_entry(g, bm + 5, 3, 20, False, False)  # two tiles
    mid = n1 // 2
    for lst, x in zip((a, b, c), big):
        lst.insert(mid, x)
    want = single(tier, *big, 1.0, 0.0, False, False)[0]
    ops.sgemm_grouped(tier, a, b, c, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(c_all, a_all * b_all)
    assert torch.equal(c[mid], want)


def test_plan_reuse():
    """Two run() calls of one plan with different alpha and beta give the
    bits of two one-shot calls."""
    tier = "wide"
    shapes = [(33, 129, 40), (1, 1, 1), (40, 0, 3), (31, 7, 100)]
    for fused in (False, True):
        a, b, c = make_group(shapes, True, True, seed=61)
        c2 = [x.clone() for x in c]
        plan = ops.GroupedPlan(tier, a, b, c, fused=fused, trans_a=True,
                               trans_b=True)
        call = ops.ft_sgemm_grouped if fused else ops.sgemm_grouped
        kw = dict(inject=False) if fused else {}
        for alpha, beta in ((1.0, 0.0), (-0.75, 1.25)):
            plan.run(alpha, beta)
            call(tier, a, b, c2, alpha, beta, trans_a=True, trans_b=True,
                 **kw)
            torch.cuda.synchronize()
            for e in range(len(shapes)):
                assert torch.equal(c[e], c2[e]), (fused, alpha, e)
