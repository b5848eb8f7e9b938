"""Fault report of the fused-ABFT kernels, on the device.

The classic kernel's injector is deterministic, so the log it leaves is
compared EXACTLY against ops.predict_injected_events (non-square shapes and
the 16-window rotation over all four waves of the huge tier catch a swapped
i/j or a dropped wave offset).  The stream-K split depends on the device's
CU count, so there the events are checked against the injector's victim-site
set instead.  What the injector cannot reach — faults away from acc[0][0][0],
the two-faults-in-one-column fail-safe, a tripped verify that locates
nothing — goes through locate_selftest_report.

Magnitude tolerance: the logged magnitude is rc, the value subtracted from
the faulty accumulator, so the error left in C is exactly rc - inj_mag; the
existing suites already hold C to ABS_TOL = 1e-2, and that is the bound used
for |rc - ERROR_INJECT| here.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import ERROR_INJECT, TIERS, TILING
from ft_sgemm_amd.ops import fault_report as fr

ABS_TOL = 1e-2
REL_TOL = 1e-2
K = 256
AMP = 0.9 * 16  # tests/test_gpu_locate_selftest.py
TAU = 9500.0

SHAPES = {"huge": (4, 2, 32), "tall": (2, 1, 32), "large_wide": (1, 2, 32),
          "medium": (1, 1, 32), "small": (1, 1, 16)}


def check(ref, got):  # tests/test_gpu_locate_e2e.py
    diff = (ref - got).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


class _streamk:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        os.environ["FT_SGEMM_STREAMK"] = self.mode

    def __exit__(self, *exc):
        os.environ.pop("FT_SGEMM_STREAMK", None)


_operands = {}


def operands(m, n):
    """(a, b, torch reference) per shape, computed once and never written."""
    if (m, n) not in _operands:
        a, b, c = ops.make_operands(m, n, K)
        _operands[(m, n)] = (a, b, ops.torch_reference(a, b, c, 1.0, 0.0))
    return _operands[(m, n)]


def run(tier, m, n, inject=True, report=None):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    a, b, _ = operands(m, n)
    c = torch.zeros((n, m), device="cuda")
    ops.ft_sgemm(tier, a, b, c, 1.0, 0.0, inject=inject, report=report)
    return c


def key(e):
    return (e.i, e.j, e.k_begin, e.k_end, e.status)


def check_magnitudes(events):
    worst = max(abs(e.magnitude - ERROR_INJECT) for e in events)
    print(f"max |rc - inj_mag| = {worst:.3e}")
    assert worst <= ABS_TOL


@pytest.mark.parametrize("tiles_m", [1, 2])
@pytest.mark.parametrize("tier", TIERS)
def test_exact_injected_events(tier, tiles_m):
    m, n = tiles_m * TILING[tier]["bm"], TILING[tier]["bn"]
    want = ops.predict_injected_events(tier, m, n, K)
    rep = ops.FaultReport()
    with _streamk("0"):
        c = run(tier, m, n, report=rep)
    r = rep.read()
    assert [key(e) for e in r.events] == [key(e) for e in want]
    assert r.tripped == r.corrected == len(r.events) == len(want)
    assert (r.uncorrected, r.unlocated, r.dropped) == (0, 0, 0)
    for got, exp in zip(r.events, want):
        assert (got.band_row, got.band_rows) == (exp.band_row, exp.band_rows)
    check_magnitudes(r.events)
    check(operands(m, n)[2], c)
    rep.raise_if_uncorrected()


@pytest.mark.parametrize("tier", TIERS)
def test_clean_run_logs_nothing(tier):
    m, n = 2 * TILING[tier]["bm"], TILING[tier]["bn"]
    rep = ops.FaultReport()
    with _streamk("0"):
        c = run(tier, m, n, inject=False, report=rep)
    r = rep.read()
    assert (r.tripped, r.corrected, r.uncorrected, r.unlocated, r.dropped,
            r.n_events) == (0, 0, 0, 0, 0, 0)
    assert r.events == []
    check(operands(m, n)[2], c)


@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("tier", TIERS)
def test_report_has_no_effect_on_c(tier, inject):
    m, n = 2 * TILING[tier]["bm"], TILING[tier]["bn"]
    modes = ["0", "1"] if TILING[tier].get("streamk") else ["0"]
    for mode in modes:
        with _streamk(mode):
            c0 = run(tier, m, n, inject=inject)
            c1 = run(tier, m, n, inject=inject, report=ops.FaultReport())
        assert torch.equal(c0, c1), f"stream-K mode {mode}"


def test_accumulate_and_reset():
    t = TILING["huge"]
    m, n = 2 * t["bm"], t["bn"]
    rep = ops.FaultReport()
    with _streamk("0"):
        run("huge", m, n, report=rep)
        once = rep.read()
        run("huge", m, n, report=rep)
        twice = rep.read()
    assert once.tripped == 32
    for f in ("tripped", "corrected", "uncorrected", "unlocated", "n_events"):
        assert getattr(twice, f) == 2 * getattr(once, f), f
    assert len(twice.events) == 2 * len(once.events)
    assert sorted(key(e) for e in twice.events) == sorted(
        2 * [key(e) for e in once.events])
    rep.reset()
    r = rep.read()
    assert (r.tripped, r.corrected, r.uncorrected, r.unlocated, r.n_events,
            r.dropped, r.events) == (0, 0, 0, 0, 0, 0, [])


def test_overflow_drops_events_but_counts_them():
    t = TILING["large"]
    m, n = 2 * t["bm"], 2 * t["bn"]
    want = {key(e) for e in ops.predict_injected_events("large", m, n, K)}
    assert len(want) == 4 * 32
    rep = ops.FaultReport(capacity=8)
    with _streamk("0"):
        c = run("large", m, n, report=rep)
    r = rep.read()
    assert r.n_events == r.corrected == r.tripped == len(want)
    assert len(r.events) == 8 and r.dropped == len(want) - 8
    assert all(key(e) in want for e in r.events)
    assert len({key(e) for e in r.events}) == 8
    check(operands(m, n)[2], c)


@pytest.mark.parametrize("tiles_m", [1, 2])
@pytest.mark.parametrize("tier", ["huge", "large"])
def test_streamk_events(tier, tiles_m):
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    mm = 32
    m, n = tiles_m * bm, bn
    sites = {(wi * wm + 4 * sub, wj * wn + r)
             for wi in range(bm // wm) for wj in range(bn // wn)
             for sub in range(64 // mm) for r in range(mm)}
    rep = ops.FaultReport()
    with _streamk("1"):
        c = run(tier, m, n, report=rep)
    r = rep.read()
    assert (r.uncorrected, r.unlocated, r.dropped) == (0, 0, 0)
    assert r.tripped == r.corrected == len(r.events) >= tiles_m
    for e in r.events:
        assert e.status == fr.STATUS_CORRECTED
        assert 0 <= e.i < m and 0 <= e.j < n
        assert (e.i % bm, e.j % bn) in sites, e
        assert 0 <= e.k_begin < e.k_end <= K and e.k_begin % 64 == 0, e
        assert e.band_row == e.i // wm * wm and e.band_rows == wm
    check_magnitudes(r.events)
    check(operands(m, n)[2], c)


# ---- self-test: the cases the injector cannot reach ----

def _site(row, col, mm):
    """(reg, lane) of fragment element (row, col): the inverse of the MFMA
    accumulator layout row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane // mm),
    col = lane % mm."""
    nreg = 16 if mm == 32 else 4
    for reg in range(nreg):
        for sub in range(64 // mm):
            if (reg & 3) + 8 * (reg >> 2) + 4 * sub == row:
                return reg, col + mm * sub
    raise AssertionError(row)


def _acc_row(reg, sub):
    return (reg & 3) + 8 * (reg >> 2) + 4 * sub


def _descs(rows):
    idesc, fdesc = ops.selftest_descriptors(rows)
    return torch.from_numpy(idesc).cuda(), torch.from_numpy(fdesc).cuda()


@pytest.mark.parametrize("name", list(SHAPES))
def test_selftest_report(name):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    fm_n, fn_n, mm = SHAPES[name]
    nreg = 16 if mm == 32 else 4
    mag = 10000.0

    # (a) one fault in the last fragment, highest register
    a_lane = 45
    a_site = (fm_n - 1, fn_n - 1, nreg - 1, a_lane)
    a_ij = ((fm_n - 1) * mm + _acc_row(nreg - 1, a_lane // mm),
            (fn_n - 1) * mm + a_lane % mm)
    # (b) +2e4 at fragment row 0 and -1e4 at fragment row 8 of column 5:
    # rc = 1e4 > tau, rw = 0 * 2e4 + 8 * (-1e4), rw / rc = -8 -> no row
    b_rc, b_rw = 2e4 - 1e4, 0 * 2e4 + 8 * -1e4
    assert b_rc > TAU and round(b_rw / b_rc) == -8
    b0, b1 = _site(0, 5, mm), _site(8, 5, mm)
    assert b0 != b1 and b0[1] % mm == b1[1] % mm == 5
    # (c) two faults in different columns
    c0, c1 = _site(3, 2, mm), _site(6, 11, mm)
    rows = [
        ([a_site + (mag,)], TAU),
        ([(0, 0) + b0 + (2e4,), (0, 0) + b1 + (-1e4,)], TAU),
        ([(0, 0) + c0 + (mag,), (fm_n - 1, fn_n - 1) + c1 + (-mag,)], TAU),
        ([(0, 0, 0, 7, TAU / 4)], TAU),
    ]
    idesc, fdesc = _descs(rows)
    tiles, counters, events = ops.locate_selftest_report(fm_n, fn_n, mm,
                                                         idesc, fdesc, AMP)
    old = ops.locate_selftest(fm_n, fn_n, mm, idesc, fdesc, AMP)
    torch.cuda.synchronize()
    shipped, clean = old[0], old[2]
    res = [fr.decode(counters[i], events[i]) for i in range(len(rows))]
    for r in res:
        assert r.tripped == 1 and r.dropped == 0

    def restored(i):
        diff = (tiles[i] - clean[i]).abs()
        rel = diff / clean[i].abs().clamp_min(1e-30)
        return not ((diff > ABS_TOL) & (rel > REL_TOL)).any()

    # the report twin corrects exactly as the shipped function does
    assert torch.equal(tiles.view(torch.int32), shipped.view(torch.int32))

    ra, rb, rc_, rd = res
    assert (ra.corrected, ra.uncorrected, ra.unlocated) == (1, 0, 0)
    (ea,) = ra.events
    assert (ea.i, ea.j) == a_ij and ea.corrected
    assert (ea.k_begin, ea.k_end, ea.band_row, ea.band_rows) == (
        0, 0, 0, fm_n * mm)
    assert abs(ea.magnitude - mag) <= ABS_TOL
    assert restored(0)

    assert (rb.corrected, rb.uncorrected, rb.unlocated) == (0, 1, 0)
    (eb,) = rb.events
    assert eb.i == -1 and eb.j == 5 and eb.status == fr.STATUS_UNCORRECTED
    assert (eb.band_row, eb.band_rows) == (0, fm_n * mm)
    assert abs(eb.magnitude - 1e4) <= ABS_TOL
    assert torch.equal(tiles[1].view(torch.int32),
                       shipped[1].view(torch.int32))
    assert not restored(1)  # the corruption is still there, and reported
    with pytest.raises(RuntimeError):
        rep = ops.FaultReport(capacity=4)
        rep.counters.copy_(counters[1])
        rep.events.copy_(events[1])
        rep.raise_if_uncorrected()

    assert (rc_.corrected, rc_.uncorrected, rc_.unlocated) == (2, 0, 0)
    assert [(e.i, e.j) for e in rc_.events] == sorted(
        [(3, 2), ((fm_n - 1) * mm + 6, (fn_n - 1) * mm + 11)])
    assert sorted(round(e.magnitude) for e in rc_.events) == [-mag, mag]
    assert restored(2)

    assert (rd.corrected, rd.uncorrected, rd.unlocated) == (0, 0, 1)
    assert rd.events == [] and rd.n_events == 0
