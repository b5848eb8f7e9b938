"""Fault report of the fused-ABFT kernels.

The fused kernels detect, locate and correct accumulator faults in
registers.  A FaultReport is the caller-owned log they fill while doing so
(layout: csrc/fault_log.h): counters, and one event per detected fault with
the element of C, the k range the fault was absorbed in, whether it could be
corrected, and the magnitude that was (or would have been) subtracted.

predict_injected_events() is the executable specification of what the
classic kernel's deterministic injector must produce; it runs on the CPU.
predict_injection_model() follows the same injections through the verify
threshold: what trips, what is corrected, and what stays in C.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List, NamedTuple

import torch

from ..kernel_table import ERROR_INJECT, TILING, threads

# csrc/fault_log.h
N_COUNTERS = 5
(C_N_EVENTS, C_TRIPPED, C_CORRECTED, C_UNCORRECTED, C_UNLOCATED) = range(5)
EVENT_DWORDS = 8
STATUS_CORRECTED = 1
STATUS_UNCORRECTED = 2


class FaultEvent(NamedTuple):
    """One detected fault.  (i, j) is the element of C (column-major M x N:
    row i, column j); for an uncorrected fault no row is known, i is -1 and
    the fault lies in rows [band_row, band_row + band_rows) of column j."""
    i: int
    j: int
    k_begin: int
    k_end: int
    status: int
    magnitude: float
    band_row: int
    band_rows: int

    @property
    def corrected(self) -> bool:
        return self.status == STATUS_CORRECTED


@dataclass
class FaultCounts:
    """Host snapshot of a FaultReport."""
    tripped: int = 0      # waves whose verify tripped
    corrected: int = 0    # faults located and corrected
    uncorrected: int = 0  # faults detected whose row fell outside the tile
    unlocated: int = 0    # tripped verifies in which no column was bad
    dropped: int = 0      # events beyond the report's capacity
    n_events: int = 0     # corrected + uncorrected, dropped ones included
    events: List[FaultEvent] = field(default_factory=list)


def _bits_to_float(v: int) -> float:
    return struct.unpack("<f", struct.pack("<i", v))[0]


def decode(counters: torch.Tensor, events: torch.Tensor) -> FaultCounts:
    """Decode a raw (counters, events) pair; one device->host copy each."""
    cnt = counters.to("cpu").tolist()
    capacity = events.shape[0]
    n = cnt[C_N_EVENTS]
    rows = events[:max(0, min(n, capacity))].to("cpu").tolist()
    evs = [FaultEvent(r[0], r[1], r[2], r[3], r[4], _bits_to_float(r[5]),
                      r[6], r[7]) for r in rows]
    evs.sort(key=lambda e: (e.i, e.j, e.k_begin))
    return FaultCounts(tripped=cnt[C_TRIPPED], corrected=cnt[C_CORRECTED],
                       uncorrected=cnt[C_UNCORRECTED],
                       unlocated=cnt[C_UNLOCATED],
                       dropped=max(0, n - capacity), n_events=n, events=evs)


class FaultReport:
    """Caller-owned fault log for ops.ft_sgemm(..., report=...).

    Owns the two int32 device tensors the kernels write.  A report
    accumulates across launches until reset(); when more than `capacity`
    events arrive the extra ones are counted (read().dropped) but not kept.

    Ragged launches (ops.ft_sgemm_ragged) compute on whole tiles whose
    out-of-range part is zero padding.  A fault absorbed there is detected,
    located and corrected like any other and its event carries its true
    padded coordinates: i >= M or j >= N is possible, and k_end is a whole
    number of panels and may exceed K.  Such an element is not part of C.
    """

    def __init__(self, capacity: int = 1024, device="cuda"):
        if capacity < 1:
            raise ValueError("FaultReport: capacity must be >= 1")
        self.capacity = int(capacity)
        self.counters = torch.zeros(N_COUNTERS, dtype=torch.int32,
                                    device=device)
        self.events = torch.zeros((self.capacity, EVENT_DWORDS),
                                  dtype=torch.int32, device=device)

    def reset(self) -> None:
        """Zero the log on the device, in stream order (no host sync)."""
        self.counters.zero_()
        self.events.zero_()

    def read(self) -> FaultCounts:
        """Synchronise once and return the counts and the sorted events."""
        if self.counters.is_cuda:
            torch.cuda.synchronize(self.counters.device)
        return decode(self.counters, self.events)

    def raise_if_uncorrected(self) -> None:
        """Refuse a result that could not be repaired."""
        r = self.read()
        if r.uncorrected or r.unlocated:
            raise RuntimeError(
                f"fused ABFT: {r.uncorrected} uncorrected and {r.unlocated} "
                f"unlocated fault(s) of {r.tripped} tripped verifies — the "
                f"result holds corruption that was detected but not repaired")


class BatchedFaultReport:
    """Caller-owned fault logs for ops.ft_sgemm_batched(..., report=...):
    one FaultReport-shaped log per batch entry, in the two tensors the
    batched kernels write — counters (batch, 5) and events (batch, capacity,
    8), int32.  Entry i of the batch reports into slot i and nowhere else.
    Accumulates across launches until reset(), like FaultReport."""

    def __init__(self, batch: int, capacity: int = 1024, device="cuda"):
        if batch < 1:
            raise ValueError("BatchedFaultReport: batch must be >= 1")
        if capacity < 1:
            raise ValueError("BatchedFaultReport: capacity must be >= 1")
        self.batch = int(batch)
        self.capacity = int(capacity)
        self.counters = torch.zeros((self.batch, N_COUNTERS),
                                    dtype=torch.int32, device=device)
        self.events = torch.zeros((self.batch, self.capacity, EVENT_DWORDS),
                                  dtype=torch.int32, device=device)

    def reset(self) -> None:
        """Zero every log on the device, in stream order (no host sync)."""
        self.counters.zero_()
        self.events.zero_()

    def read(self) -> List[FaultCounts]:
        """Synchronise once and return one FaultCounts per batch entry."""
        if self.counters.is_cuda:
            torch.cuda.synchronize(self.counters.device)
        counters, events = self.counters.to("cpu"), self.events.to("cpu")
        return [decode(counters[i], events[i]) for i in range(self.batch)]

    def raise_if_uncorrected(self) -> None:
        """Refuse a batch in which some entry could not be repaired."""
        bad = [(i, r) for i, r in enumerate(self.read())
               if r.uncorrected or r.unlocated]
        if bad:
            detail = ", ".join(
                f"entry {i}: {r.uncorrected} uncorrected, {r.unlocated} "
                f"unlocated of {r.tripped} tripped" for i, r in bad)
            raise RuntimeError(
                f"fused ABFT (batched): batch entries "
                f"{[i for i, _ in bad]} hold corruption that was detected "
                f"but not repaired ({detail})")


def predict_injected_events(tier: str, m: int, n: int, k: int,
                            verify_windows: int = 20,
                            ragged: bool = False,
                            streamk_grid: int = 0) -> List[FaultEvent]:
    """The exact events the classic fused kernel's injector must produce for
    an (m, n, k) GEMM on `tier`, sorted by (i, j, k_begin).

    Derived from csrc/tier_launch.hpp (window_stride as launch_tier calls
    it) and csrc/ft_kernels.hpp (sgemm_mfma: victim rotation, MFMA
    accumulator layout): every block injects once per verify window w into
    acc[0][0][0] of thread (w * 67) % THREADS.

    ragged: model ft_sgemm_ragged (csrc/ft_ragged.hpp) instead: any shape, a
    ceil(m/bm) x ceil(n/bn) grid and ceil(k/bkf) panels, the same rule in
    every block.  In an edge tile a victim can lie in the padding (i >= m
    or j >= n), and the last window's k_end is a whole number of panels and
    can exceed k: both are predicted as the kernel logs them.

    streamk_grid > 0 (with ragged): model ft_sgemm_ragged(..., streamk=grid)
    (csrc/ft_ragged_streamk.hpp) instead.  Every segment of
    ragged_streamk_partition injects once per group of `stride` units counted
    from its own start, stride = max(1, ceil(k/64) // verify_windows), into
    acc[0][0][0] of thread ((w_lo + g*stride) * 67 + tile * 13) % THREADS; the
    group's k range starts at 64 * (w_lo + g*stride) and ends after its last
    whole panel.
    """
    if streamk_grid:
        if not ragged:
            raise ValueError("streamk_grid needs ragged=True")
        return _predict_streamk_events(tier, m, n, k, verify_windows,
                                       streamk_grid)
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    bkf = t.get("bkf", t["bk"])
    mm = 16 if t["mfma"] == "f32_16x16x4" else 32
    if ragged:
        if min(m, n, k) < 1:
            raise ValueError(f"shape ({m}, {n}, {k}) is empty")
    elif m % bm or n % bn or k % bkf:
        raise ValueError(f"shape ({m}, {n}, {k}) does not divide tier {tier}")
    nthreads = threads(tier)
    waves_n = bn // wn
    niter = -(-k // bkf)
    stride = max(1, niter // (verify_windows if verify_windows > 0 else 20))
    nwin = -(-niter // stride)
    out = []
    for bx in range(-(-m // bm)):
        for by in range(-(-n // bn)):
            for w in range(nwin):
                tid = (w * 67) % nthreads
                wave, lane = tid >> 6, tid & 63
                sub, r = lane // mm, lane % mm
                out.append(FaultEvent(
                    i=bx * bm + (wave // waves_n) * wm + 4 * sub,
                    j=by * bn + (wave % waves_n) * wn + r,
                    k_begin=w * stride * bkf,
                    k_end=min((w + 1) * stride, niter) * bkf,
                    status=STATUS_CORRECTED, magnitude=ERROR_INJECT,
                    band_row=bx * bm + (wave // waves_n) * wm,
                    band_rows=wm))
    out.sort(key=lambda e: (e.i, e.j, e.k_begin))
    return out


def _predict_streamk_events(tier, m, n, k, verify_windows, grid):
    from .ragged_streamk import ragged_streamk_partition
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    bkf = t.get("bkf", t["bk"])
    mm = 16 if t["mfma"] == "f32_16x16x4" else 32
    nthreads = threads(tier)
    waves_n = bn // wn
    upt = -(-k // 64)
    stride = max(1, upt // (verify_windows if verify_windows > 0 else 20))
    out = []
    for segs in ragged_streamk_partition(tier, m, n, k, grid, True)[0]:
        for tile, bx, by, w_lo, w_hi, _ in segs:
            kbase = 64 * w_lo
            npan = -(-(min(k, 64 * w_hi) - kbase) // bkf)
            for u0 in range(w_lo, w_hi, stride):
                tid = (u0 * 67 + tile * 13) % nthreads
                wave, lane = tid >> 6, tid & 63
                sub, r = lane // mm, lane % mm
                p_end = min((u0 - w_lo + stride) * (64 // bkf), npan)
                out.append(FaultEvent(
                    i=bx * bm + (wave // waves_n) * wm + 4 * sub,
                    j=by * bn + (wave % waves_n) * wn + r,
                    k_begin=64 * u0, k_end=kbase + p_end * bkf,
                    status=STATUS_CORRECTED, magnitude=ERROR_INJECT,
                    band_row=bx * bm + (wave // waves_n) * wm,
                    band_rows=wm))
    out.sort(key=lambda e: (e.i, e.j, e.k_begin))
    return out


def predict_injected_events_grouped(tier: str, shapes,
                                    verify_windows: int = 20,
                                    streamk_grid: int = 0
                                    ) -> List[List[FaultEvent]]:
    """Per entry of a grouped fused launch on `tier`, the exact events its
    injector must produce, each list sorted by (i, j, k_begin).  shapes:
    (m, n, k, ...) per entry, as grouped_layout returns them.

    streamk_grid == 0 models ft_sgemm_grouped's classic launch: entry e has
    the events of ft_sgemm_ragged on its own shape, an empty entry none.

    streamk_grid > 0 models ft_sgemm_grouped(..., streamk=grid)
    (csrc/ft_ragged_grouped_streamk.hpp).  Every segment of
    grouped_streamk_partition injects once per group of stride_e units
    counted from its own start, stride_e = max(1, upt_e // verify_windows),
    into acc[0][0][0] of thread ((w_lo + g*stride_e) * 67 + tile * 13) %
    THREADS with `tile` the entry-local tile index; a segment of a k == 0
    entry has no panels and injects nothing.  Coordinates are the entry's
    own."""
    if not streamk_grid:
        return [predict_injected_events(tier, s[0], s[1], s[2],
                                        verify_windows, ragged=True)
                if min(s[:3]) > 0 else [] for s in shapes]
    from .grouped_streamk import grouped_streamk_partition
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    bkf = t.get("bkf", t["bk"])
    mm = 16 if t["mfma"] == "f32_16x16x4" else 32
    nthreads = threads(tier)
    waves_n = bn // wn
    windows = verify_windows if verify_windows > 0 else 20
    out = [[] for _ in shapes]
    for segs in grouped_streamk_partition(tier, shapes, streamk_grid)[0]:
        for e, tile, bx, by, w_lo, w_hi, _ in segs:
            k = shapes[e][2]
            if k == 0:
                continue
            stride = max(1, -(-k // 64) // windows)
            kbase = 64 * w_lo
            npan = -(-(min(k, 64 * w_hi) - kbase) // bkf)
            for u0 in range(w_lo, w_hi, stride):
                tid = (u0 * 67 + tile * 13) % nthreads
                wave, lane = tid >> 6, tid & 63
                sub, r = lane // mm, lane % mm
                p_end = min((u0 - w_lo + stride) * (64 // bkf), npan)
                out[e].append(FaultEvent(
                    i=bx * bm + (wave // waves_n) * wm + 4 * sub,
                    j=by * bn + (wave % waves_n) * wn + r,
                    k_begin=64 * u0, k_end=kbase + p_end * bkf,
                    status=STATUS_CORRECTED, magnitude=ERROR_INJECT,
                    band_row=bx * bm + (wave // waves_n) * wm,
                    band_rows=wm))
    for ev in out:
        ev.sort(key=lambda x: (x.i, x.j, x.k_begin))
    return out


class InjectionModel(NamedTuple):
    """What the classic fused kernel must do with its injector's faults for
    a given (tau, inj_mag); see predict_injection_model."""
    mult: torch.Tensor     # (m, n) int32: injections per element of C
    residue: torch.Tensor  # (m, n) fp64: injected magnitude left in the
    #                        accumulators (before the alpha/beta epilogue)
    tripped: int           # verifies whose wave residual exceeded tau
    corrected: int
    uncorrected: int
    unlocated: int         # tripped verifies in which no column was bad
    n_faults: int          # corrected + uncorrected: the event count
    wave_totals: dict      # (bx, by, wave) -> peak |running residual|
    col_totals: dict       # (bx, by, wave, column) -> peak |running residual|


def predict_injection_model(tier: str, m: int, n: int, k: int, tau: float,
                            inj_mag: float, verify_windows: int = 20,
                            ragged: bool = False) -> InjectionModel:
    """CPU model of inject -> verify -> locate -> correct in the classic
    fused kernel, from the same rotation rule as predict_injected_events.

    Every block injects inj_mag once per verify window w into acc[0][0][0]
    of thread (w * 67) % THREADS; at the end of each window every wave
    compares its whole tile's residual (the running total of what was
    injected into it and not corrected yet) against tau.  A wave that trips
    looks at each of its columns: a column whose own total exceeds tau is a
    fault of that magnitude at row round(sum(row * e) / sum(e)), corrected
    when that row lies in the wave tile; when no column exceeds tau the
    verify is counted as unlocated and the accumulators stay as they are.
    Roundoff (orders of magnitude below any tau in use) is not modelled.

    ragged: model ft_sgemm_ragged: any shape, ceil grids and ceil(k/bkf)
    panels.  The counts cover every block, padding victims included; mult
    and residue are the (m, n) window of C, where padding never lands.
    """
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    bkf = t.get("bkf", t["bk"])
    mm = 16 if t["mfma"] == "f32_16x16x4" else 32
    if ragged:
        if min(m, n, k) < 1:
            raise ValueError(f"shape ({m}, {n}, {k}) is empty")
    elif m % bm or n % bn or k % bkf:
        raise ValueError(f"shape ({m}, {n}, {k}) does not divide tier {tier}")
    nthreads = threads(tier)
    nwaves = nthreads // 64
    waves_n = bn // wn
    niter = -(-k // bkf)
    gx, gy = -(-m // bm), -(-n // bn)
    stride = max(1, niter // (verify_windows if verify_windows > 0 else 20))
    nwin = -(-niter // stride)
    tripped = corrected = uncorrected = unlocated = 0
    wave_totals, col_totals = {}, {}
    # one block's history is every block's: simulate one, then tile it
    pending = [dict() for _ in range(nwaves)]  # col -> {row: magnitude}
    bmult = torch.zeros((bm, bn), dtype=torch.int32)
    wave_peak = [0.0] * nwaves
    col_peak = {}
    for w in range(nwin):
        tid = (w * 67) % nthreads
        wave, lane = tid >> 6, tid & 63
        row, col = 4 * (lane // mm), lane % mm
        rows = pending[wave].setdefault(col, {})
        rows[row] = rows.get(row, 0.0) + inj_mag
        bmult[(wave // waves_n) * wm + row, (wave % waves_n) * wn + col] += 1
        for wv in range(nwaves):
            total = sum(sum(r.values()) for r in pending[wv].values())
            wave_peak[wv] = max(wave_peak[wv], abs(total))
            for c, r in pending[wv].items():
                key = (wv, c)
                col_peak[key] = max(col_peak.get(key, 0.0),
                                    abs(sum(r.values())))
            if not abs(total) > tau:
                continue
            tripped += 1
            any_bad = False
            for c, r in pending[wv].items():
                rc = sum(r.values())
                if not abs(rc) > tau:
                    continue
                any_bad = True
                at = int(round(sum(i * e for i, e in r.items()) / rc))
                if 0 <= at < wm:
                    corrected += 1
                    r[at] = r.get(at, 0.0) - rc
                else:
                    uncorrected += 1
            if not any_bad:
                unlocated += 1
    bres = torch.zeros((bm, bn), dtype=torch.float64)
    for wv in range(nwaves):
        for c, r in pending[wv].items():
            for i, e in r.items():
                bres[(wv // waves_n) * wm + i, (wv % waves_n) * wn + c] += e
    nblk = gx * gy
    mult = bmult.repeat(gx, gy)[:m, :n]
    residue = bres.repeat(gx, gy)[:m, :n]
    for bx in range(gx):
        for by in range(gy):
            for wv in range(nwaves):
                wave_totals[(bx, by, wv)] = wave_peak[wv]
            for (wv, c), v in col_peak.items():
                col_totals[(bx, by, wv, c)] = v
    return InjectionModel(mult=mult, residue=residue,
                          tripped=tripped * nblk, corrected=corrected * nblk,
                          uncorrected=uncorrected * nblk,
                          unlocated=unlocated * nblk,
                          n_faults=(corrected + uncorrected) * nblk,
                          wave_totals=wave_totals, col_totals=col_totals)
