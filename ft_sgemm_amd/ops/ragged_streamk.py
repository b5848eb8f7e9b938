"""Stream-K for the single ragged launch: the CPU-runnable side.

ragged_streamk_partition() mirrors the work walk of
sgemm_mfma_ragged_streamk (csrc/ft_ragged_streamk.hpp); the tests and the
injector predictor (fault_report.predict_injected_events) are built on it.
ragged_streamk_layout() is the mirror of the launch rules gemm_args_error
states for sk_grid > 0.  ragged_streamk_gate() says where stream-K is
expected to win; RAGGED_STREAMK_NOTE says what that rests on.  Nothing here
touches the extension.
"""

from __future__ import annotations

import torch

from ..kernel_table import TILING

UNIT_K = 64  # one work unit: a 64-k window of one output tile


def has_streamk(tier: str) -> bool:
    """Does `tier` have stream-K twins (kernel_table.py streamk)?"""
    return bool(TILING[tier].get("streamk", False))


def ragged_streamk_units(tier: str, m: int, n: int, k: int):
    """(tiles along M, tiles along N, units per tile) of an (m, n, k) ragged
    product on `tier`: ceil counts, the last unit of a tile short when
    k % 64 != 0."""
    t = TILING[tier]
    if min(m, n, k) < 1:
        raise ValueError(f"shape ({m}, {n}, {k}) is empty")
    return -(-m // t["bm"]), -(-n // t["bn"]), -(-k // UNIT_K)


def ragged_streamk_partition(tier: str, m: int, n: int, k: int, grid: int,
                             fused: bool = False):
    """The kernel's partition of an (m, n, k) product over `grid` workgroups.

    Returns (segments, grid): the grid clamped to the unit count, and per
    workgroup, in the order it runs them, its segments
    (tile, bx, by, w_lo, w_hi, kind).  tile = bx + by * ceil(m / bm); the
    segment covers units [w_lo, w_hi) of that tile, i.e.
    k in [64 * w_lo, min(k, 64 * w_hi)).  kind is "full" when the workgroup
    owns the whole tile (it takes the epilogue itself), "tail" when the
    segment starts the tile and leaves its end to later workgroups (partial
    slot 2g + 1), "head" otherwise (slot 2g): a tile's segments are one tail,
    then heads, in workgroup order, which is the order the fixup pass sums
    them in.

    The units are the same for the plain and the fused kernel (the fused
    panel depth divides 64), so `fused` does not change the result; it is
    taken so that callers can pass what they launch."""
    del fused
    if not has_streamk(tier):
        raise ValueError(f"tier {tier} has no stream-K twin")
    if grid < 1:
        raise ValueError(f"grid {grid} must be >= 1")
    ntm, ntn, upt = ragged_streamk_units(tier, m, n, k)
    total = ntm * ntn * upt
    grid = min(grid, total)
    q, rem = divmod(total, grid)
    out = []
    for wg in range(grid):
        u = wg * q + min(wg, rem)
        u_end = u + q + (1 if wg < rem else 0)
        segs = []
        while u < u_end:
            tile = u // upt
            w_lo = u - tile * upt
            w_hi = w_lo + min(u_end - u, upt - w_lo)
            kind = ("full" if w_lo == 0 and w_hi == upt
                    else "tail" if w_lo == 0 else "head")
            segs.append((tile, tile % ntm, tile // ntm, w_lo, w_hi, kind))
            u += w_hi - w_lo
        out.append(segs)
    return out, grid


def streamk_partials_floats(tier: str, grid: int) -> int:
    """Floats of the partials buffer of a stream-K launch on `grid`
    workgroups: a head and a tail slot of bm x bn each."""
    t = TILING[tier]
    return 2 * grid * t["bm"] * t["bn"]


def ragged_streamk_layout(tier: str, m: int, n: int, k: int, grid: int,
                          partials: torch.Tensor | None = None) -> int:
    """Validate the stream-K arguments of a ragged call and return the
    clamped grid.  Runs on any device: the CPU-runnable mirror of what
    gemm_args_error (csrc/dispatch.hip) asks of sk_grid > 0.  The tier must
    have a stream-K twin; partials, when given, must be a contiguous fp32
    tensor of at least streamk_partials_floats(tier, clamped grid) elements,
    16-byte aligned.  Raises ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_ragged(streamk): {msg}")

    if not has_streamk(tier):
        err(f"tier {tier} has no stream-K twin")
    if grid < 1:
        err(f"grid {grid} must be >= 1")
    ntm, ntn, upt = ragged_streamk_units(tier, m, n, k)
    if ntm * ntn * upt > 2**31 - 1:
        err("more than 2^31 - 1 work units")
    grid = min(grid, ntm * ntn * upt)
    if partials is not None:
        need = streamk_partials_floats(tier, grid)
        if partials.dtype != torch.float32 or not partials.is_contiguous():
            err("partials must be a contiguous float32 tensor")
        if partials.numel() < need:
            err(f"partials holds {partials.numel()} floats, a grid of "
                f"{grid} needs {need}")
        if partials.data_ptr() % 16:
            err("partials must be 16-byte aligned")
    return grid


# The device grid the measured runs had (profiles/ragged_streamk.txt): 256 CUs
# x resident workgroups of the plain kernel.  The gate runs without a device,
# so it carries the figures; the fused large kernel's grid (2048) is judged by
# the same slots.
_GATE_SLOTS = {"huge": 512, "large": 2560}
# Smallest idle share of the classic grid's last dispatch round at which
# stream-K measured faster than both classic arms.
_GATE_WASTE = {"huge": 0.35, "large": 0.90}
_GATE_MIN_K = 3073  # the shallowest K measured


def ragged_streamk_gate(tier: str, m: int, n: int, k: int,
                        fused: bool) -> bool:
    """Is stream-K on `tier` at the device grid expected to beat both the
    classic ragged launch on `tier` and the one on
    choose_tier(m, n, k, ragged=True)'s tier?  True only in regimes where it
    measured so (RAGGED_STREAMK_NOTE): the classic grid of ceil tiles leaves
    at least the tier's measured share of its last dispatch round idle, and
    K is at least the shallowest measured.  The same rule for the plain and
    the fused kernel: they won and lost in the same cells.  The explicit
    streamk= argument of sgemm_ragged / ft_sgemm_ragged works everywhere
    regardless."""
    del fused
    if not has_streamk(tier) or min(m, n, k) < 1 or k < _GATE_MIN_K:
        return False
    ntm, ntn, _ = ragged_streamk_units(tier, m, n, k)
    slots = _GATE_SLOTS[tier]
    rounds = -(-(ntm * ntn) // slots)
    waste = 1.0 - ntm * ntn / (rounds * slots)
    return waste >= _GATE_WASTE[tier]


# What ragged_streamk_gate rests on.
RAGGED_STREAMK_NOTE = (
    "measured (profiles/ragged_streamk.txt, MI355X, untransposed operands, "
    "plain and fused no-inject, arms interleaved in one process, median of 5 "
    "rounds, spreads <= 1.2%, classic-vs-classic noise <= 0.3%), stream-K at "
    "the device grid (huge 512, large 2560 plain / 2048 fused) against the "
    "better of the classic launch on the same tier and on choose_tier's "
    "tier, six cells.  grad_weight 1024x1024 with K = 16384 / 65536 and "
    "1000x1000 with K = 16385 (32 huge or 256 large tiles, choose_tier -> "
    "medium): huge stream-K 1.66-2.84x, large 1.48-2.33x; huge stream-K is "
    "the fastest arm (96-124 TF at 1024, 77-81 TF at 1000).  4097x4097x4096 "
    "(561 huge tiles on 512 slots): huge 1.34-1.35x; large 0.93-0.99x (17% "
    "of its second round idle: no win).  3073^3 (325 huge tiles; "
    "choose_tier -> large): huge 1.24-1.34x; large 0.90x plain, 1.08x "
    "fused.  Control 4096x4096x8192 (1024 huge tiles, two full rounds): "
    "huge 0.99-1.00x, large 0.77-0.78x against huge classic: no win.  The "
    "gate: K >= 3073 and the idle share of the classic grid's last round at "
    "least 35% on huge (the measured wins have 36%, 45% and 94%; 0% lost) "
    "and 90% on large (its wins have 90%; 6% and 17% did not win, fused "
    "3073^3 apart).  Extrapolated, not measured: idle shares between the "
    "measured ones, K below 3073 (False), transposed operands (ft_linear's "
    "forward and grad_x; the fused huge TT kernels spill 32 B/lane, "
    "docs/ABLATION.md section 19), launches with injection or a report, "
    "and devices whose grid differs from the measured one")
