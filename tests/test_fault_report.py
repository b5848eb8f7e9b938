"""Fault report, the parts that need no GPU: predict_injected_events (the
executable specification of the classic kernel's injector that
tests/test_gpu_fault_report.py compares the device log against) and the
decoding of a FaultReport's raw tensors."""

import struct

import pytest
import torch

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import ERROR_INJECT, TIERS, TILING
from ft_sgemm_amd.ops import fault_report as fr

K = 256


def _windows(tier, k=K, verify_windows=20):
    bkf = TILING[tier].get("bkf", TILING[tier]["bk"])
    niter = k // bkf
    stride = max(1, niter // verify_windows)
    return bkf, niter, stride, -(-niter // stride)


@pytest.mark.parametrize("tier", TIERS)
def test_predict_injected_events(tier):
    t = TILING[tier]
    m, n = 2 * t["bm"], t["bn"]
    _, _, _, nwin = _windows(tier)
    ev = ops.predict_injected_events(tier, m, n, K)
    assert len(ev) == 2 * nwin
    keys = [(e.i, e.j, e.k_begin) for e in ev]
    assert len(set(keys)) == len(keys)
    assert keys == sorted(keys)
    for e in ev:
        assert 0 <= e.i < m and 0 <= e.j < n
        assert e.status == fr.STATUS_CORRECTED and e.corrected
        assert e.magnitude == ERROR_INJECT
        assert e.band_row <= e.i < e.band_row + e.band_rows
    # per block, the k ranges tile [0, K) without gap or overlap
    for bx in range(2):
        rng = sorted((e.k_begin, e.k_end) for e in ev
                     if e.i // t["bm"] == bx)
        assert len(rng) == nwin
        assert rng[0][0] == 0 and rng[-1][1] == K
        for (b0, e0), (b1, _) in zip(rng, rng[1:]):
            assert b0 < e0 == b1


def test_predict_huge_victims_in_all_four_waves():
    t = TILING["huge"]
    ev = ops.predict_injected_events("huge", t["bm"], t["bn"], K)
    assert len(ev) == 16
    waves = {(e.i // t["wm"], e.j // t["wn"]) for e in ev}
    assert waves == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_predict_stride_and_tail_window():
    # huge, K=1024: niter 64, stride 3 -> 22 windows, the last one short
    ev = ops.predict_injected_events("huge", 256, 128, 1024)
    assert len(ev) == 22
    last = max(ev, key=lambda e: e.k_begin)
    assert (last.k_begin, last.k_end) == (21 * 3 * 16, 1024)
    # 4 windows asked for: stride 16, four full windows
    ev4 = ops.predict_injected_events("huge", 256, 128, 1024,
                                      verify_windows=4)
    assert sorted((e.k_begin, e.k_end) for e in ev4) == [
        (0, 256), (256, 512), (512, 768), (768, 1024)]


def test_predict_rejects_undivided_shape():
    with pytest.raises(ValueError):
        ops.predict_injected_events("huge", 100, 128, K)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _fill(rep, counters, rows):
    rep.counters.copy_(torch.tensor(counters, dtype=torch.int32))
    for s, r in enumerate(rows):
        rep.events[s] = torch.tensor(r, dtype=torch.int32)


def test_report_decoding_sorts_and_bitcasts():
    rep = ops.FaultReport(capacity=4, device="cpu")
    assert rep.counters.dtype == torch.int32 and rep.counters.shape == (5,)
    assert rep.events.dtype == torch.int32 and rep.events.shape == (4, 8)
    rows = [
        [7, 3, 64, 128, 1, _bits(10000.25), 0, 128],
        [2, 9, 0, 64, 1, _bits(-9999.5), 0, 128],
        [-1, 5, 0, 64, 2, _bits(1e4), 128, 128],
        [2, 9, 0, 32, 1, _bits(1.5), 0, 128],  # beyond n_events: not read
    ]
    # {n_events, tripped, corrected, uncorrected, unlocated}
    _fill(rep, [3, 4, 2, 1, 1], rows)
    r = rep.read()
    assert (r.tripped, r.corrected, r.uncorrected, r.unlocated) == (4, 2, 1, 1)
    assert r.dropped == 0 and r.n_events == 3
    assert [(e.i, e.j, e.k_begin) for e in r.events] == [
        (-1, 5, 0), (2, 9, 0), (7, 3, 64)]
    assert [e.magnitude for e in r.events] == [1e4, -9999.5, 10000.25]
    assert [e.corrected for e in r.events] == [False, True, True]
    assert (r.events[0].band_row, r.events[0].band_rows) == (128, 128)
    assert r.events[2].k_end == 128


def test_report_dropped_and_reset():
    rep = ops.FaultReport(capacity=2, device="cpu")
    _fill(rep, [5, 5, 5, 0, 0], [[1, 1, 0, 16, 1, _bits(1e4), 0, 32],
                                 [0, 1, 0, 16, 1, _bits(1e4), 0, 32]])
    r = rep.read()
    assert r.n_events == 5 and r.dropped == 3 and len(r.events) == 2
    assert [e.i for e in r.events] == [0, 1]
    rep.raise_if_uncorrected()  # all corrected: no raise
    rep.reset()
    r = rep.read()
    assert (r.tripped, r.corrected, r.uncorrected, r.unlocated, r.dropped,
            r.n_events, r.events) == (0, 0, 0, 0, 0, 0, [])


@pytest.mark.parametrize("counters,raises", [
    ([0, 0, 0, 0, 0], False),
    ([2, 2, 2, 0, 0], False),
    ([2, 2, 1, 1, 0], True),   # an uncorrected fault
    ([0, 1, 0, 0, 1], True),   # tripped, nothing located
])
def test_raise_if_uncorrected(counters, raises):
    rep = ops.FaultReport(capacity=4, device="cpu")
    _fill(rep, counters, [])
    if raises:
        with pytest.raises(RuntimeError, match="uncorrected"):
            rep.raise_if_uncorrected()
    else:
        rep.raise_if_uncorrected()


def test_report_rejected_for_unfused_ids():
    rep = ops.FaultReport(capacity=1, device="cpu")
    for kid in (0, 6, 10):
        with pytest.raises(ValueError):
            ops.run_kernel_id(kid, None, None, None, report=rep)
