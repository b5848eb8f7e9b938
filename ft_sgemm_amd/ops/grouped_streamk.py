"""Stream-K for the grouped ragged launch: the CPU-runnable side.

grouped_streamk_partition() mirrors the work walk of
sgemm_mfma_ragged_grouped_streamk (csrc/ft_ragged_grouped_streamk.hpp); the
tests and the injector predictor
(fault_report.predict_injected_events_grouped) are built on it.
grouped_streamk_layout() is the mirror of the rules grouped_args_error
(csrc/dispatch.hip) states for sk_grid > 0 and of the binding's partials
checks.  grouped_streamk_gate() says where grouped stream-K is expected to
win; GROUPED_STREAMK_NOTE says what that rests on.  Nothing here touches the
extension.
"""

from __future__ import annotations

import torch

from ..kernel_table import TILING
from .ragged_streamk import UNIT_K, has_streamk, streamk_partials_floats

MAX_UNITS = 2 ** 31 - 1  # the unit index is an int in the kernels


def grouped_streamk_units(tier: str, shapes):
    """Per entry of `shapes` ((m, n, k, ...) each, as grouped_layout returns
    them) the triple (tiles along M, tiles along N, units per tile) on
    `tier`.  Units per tile are max(1, ceil(k / 64)): an entry with k == 0
    has one empty unit per tile, whose owner writes beta * c.  An entry with
    m == 0 or n == 0 has no tiles, hence no units."""
    t = TILING[tier]
    out = []
    for s in shapes:
        m, n, k = s[:3]
        if min(m, n, k) < 0:
            raise ValueError(f"shape ({m}, {n}, {k}) has a negative size")
        out.append((-(-m // t["bm"]), -(-n // t["bn"]),
                    max(1, -(-k // UNIT_K))))
    return out


def _total_units(units):
    return sum(ntm * ntn * upt for ntm, ntn, upt in units)


def grouped_streamk_partition(tier: str, shapes, grid: int):
    """The kernel's partition of a group over `grid` workgroups.

    Returns (segments, grid): the grid clamped to the unit count, and per
    workgroup, in the order it runs them, its segments
    (entry, tile, bx, by, w_lo, w_hi, kind).  The units are ordered by entry,
    then tile (entry-local, tile = bx + by * ceil(m / bm)), then k, and cut
    into balanced contiguous ranges, the first total % grid workgroups taking
    one extra unit; a range may cross tile and entry boundaries.  A segment
    covers units [w_lo, w_hi) of its tile, i.e. k in
    [64 * w_lo, min(k, 64 * w_hi)), which is empty for the one unit of a
    k == 0 tile.  kind is "full" when the workgroup owns the whole tile (it
    takes the epilogue itself), "tail" when the segment starts the tile and
    leaves its end to later workgroups (partial slot 2g + 1), "head"
    otherwise (slot 2g): a tile's segments are one tail, then heads, in
    workgroup order, which is the order the fixup pass sums them in.  A group
    without units returns ([], 0)."""
    if not has_streamk(tier):
        raise ValueError(f"tier {tier} has no stream-K twin")
    if grid < 1:
        raise ValueError(f"grid {grid} must be >= 1")
    units = grouped_streamk_units(tier, shapes)
    start = [0]  # unit_start: exclusive prefix of the entries' unit counts
    for ntm, ntn, upt in units:
        start.append(start[-1] + ntm * ntn * upt)
    total = start[-1]
    if total == 0:
        return [], 0
    grid = min(grid, total)
    q, rem = divmod(total, grid)
    out, e = [], 0
    for wg in range(grid):
        u = wg * q + min(wg, rem)
        u_end = u + q + (1 if wg < rem else 0)
        segs = []
        while u < u_end:
            while u >= start[e + 1]:  # entries without units are skipped
                e += 1
            ntm, _, upt = units[e]
            tile, w_lo = divmod(u - start[e], upt)
            w_hi = w_lo + min(u_end - u, upt - w_lo)
            kind = ("full" if w_lo == 0 and w_hi == upt
                    else "tail" if w_lo == 0 else "head")
            segs.append((e, tile, tile % ntm, tile // ntm, w_lo, w_hi, kind))
            u += w_hi - w_lo
        out.append(segs)
    return out, grid


def grouped_streamk_layout(tier: str, shapes, grid: int,
                           partials: torch.Tensor | None = None) -> int:
    """Validate the stream-K arguments of a grouped call and return the
    clamped grid (0 for a group without units, which launches nothing).  Runs
    on any device: the CPU-runnable mirror of what grouped_args_error
    (csrc/dispatch.hip) asks of sk_grid > 0 and of the binding's partials
    checks.  The tier must have a stream-K twin, the grid be >= 1 and the
    units at most 2^31 - 1; partials, when given, must be a contiguous fp32
    tensor of at least streamk_partials_floats(tier, clamped grid) elements,
    16-byte aligned.  Raises ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_grouped(streamk): {msg}")

    if not has_streamk(tier):
        err(f"tier {tier} has no stream-K twin")
    if grid < 1:
        err(f"grid {grid} must be >= 1")
    total = _total_units(grouped_streamk_units(tier, shapes))
    if total > MAX_UNITS:
        err("more than 2^31 - 1 work units")
    grid = min(grid, total)
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


# The device grid the measured runs had (profiles/grouped_streamk.txt): 256
# CUs x resident workgroups of the untransposed kernel.  The gate runs
# without a device, so it carries the figures.
_GATE_SLOTS = {"huge": 512, "large": 2560}
# Smallest imbalance of the classic grid at which grouped stream-K measured
# faster than both classic arms.
_GATE_IMBALANCE = {"huge": 7.0, "large": 4.3}
# huge only: the deep regime, a half-empty chip under tiles of >= 128 units
_GATE_DEEP_IMBALANCE, _GATE_DEEP_UNITS = 2.0, 128
_GATE_MAX_TILES = 1 << 17  # beyond it the chip is full whatever the counts
# Fewest units per workgroup of the device grid among the measured wins
# (huge, halving counts: 2336 units on 512 workgroups); a smaller launch is
# overhead, whatever its imbalance.
_GATE_MIN_UNITS_PER_SLOT = 4.5


def classic_imbalance(tier: str, shapes, slots: int):
    """(imbalance, mean units per tile) of the classic grouped grid of
    `shapes` on `tier` with `slots` resident workgroups.  The model: tiles
    are handed to the slots in launch order, each to the slot that frees
    first, and a tile costs its units, max(1, ceil(k / 64)); imbalance is
    the makespan over the balanced share, total units / slots.  1.0 is a
    chip that is evenly busy until the end; 8.0 a launch that takes eight
    times as long as its work shared out evenly would."""
    import heapq
    costs = [upt for ntm, ntn, upt in grouped_streamk_units(tier, shapes)
             for _ in range(ntm * ntn)]
    if not costs:
        return 0.0, 0.0
    free = [0] * min(slots, len(costs))
    for c in costs:
        heapq.heapreplace(free, free[0] + c)
    total = sum(costs)
    return max(free) * slots / total, total / len(costs)


def grouped_streamk_gate(tier: str, shapes, fused: bool) -> bool:
    """Is grouped stream-K on `tier` at the device grid expected to beat both
    the classic grouped launch on `tier` and the one on
    choose_tier_grouped(shapes)'s tier?  True only in regimes where it
    measured so (GROUPED_STREAMK_NOTE): the classic grid is at least as
    imbalanced (classic_imbalance at the measured grid) as the tier's
    shallowest measured win, or, on huge, at least half idle under tiles of
    128 units or more.  The same rule for the plain and the fused kernel:
    they won and lost in the same cells.  The explicit streamk= argument of
    GroupedPlan / sgemm_grouped / ft_sgemm_grouped works everywhere
    regardless."""
    del fused
    if not has_streamk(tier):
        return False
    units = grouped_streamk_units(tier, shapes)
    if sum(ntm * ntn for ntm, ntn, _ in units) > _GATE_MAX_TILES:
        return False
    if _total_units(units) < _GATE_MIN_UNITS_PER_SLOT * _GATE_SLOTS[tier]:
        return False
    imb, mean_upt = classic_imbalance(tier, shapes, _GATE_SLOTS[tier])
    if imb >= _GATE_IMBALANCE[tier]:
        return True
    return (tier == "huge" and imb >= _GATE_DEEP_IMBALANCE and
            mean_upt >= _GATE_DEEP_UNITS)


# What grouped_streamk_gate rests on.
GROUPED_STREAMK_NOTE = (
    "measured (profiles/grouped_streamk.txt, MI355X, in = out = 1024, plain "
    "and fused no-inject, arms interleaved in one process, median of 5 "
    "rounds, spreads <= 2.8%, classic-vs-classic noise <= 0.7%), grouped "
    "stream-K at the device grid (huge 512, large 2560; large forward 2048) "
    "against the better of the classic grouped launch on the same tier and "
    "on choose_tier_grouped's tier, seven cells.  grad_weight, 16 experts "
    "with halving counts and 4 empty (classic imbalance 7.0 on huge, 4.4 on "
    "large): huge 2.00-2.02x, large 1.13x plain and 1.35x fused; large "
    "stream-K is the fastest arm.  grad_weight, 8 experts x 8192 tokens "
    "(imbalance 2.0 on huge, tiles of 128 units): huge 1.06x, the fastest "
    "arm at 130 TF plain; large (imbalance 1.25) 0.79-0.99x.  grad_weight, "
    "8 even experts x 512 tokens (imbalance 2.0 / 1.25, tiles of 8 units): "
    "0.66-0.98x, no win: the tiles are too shallow to pay for partials and "
    "fixup.  grad_weight, 64 drawn counts (2048 huge tiles, imbalance 1.35 "
    "/ 1.14): 0.72-0.91x, no win: the chip is full.  Forward controls "
    "(both operands transposed, K = 1024): even 0.81-0.99x, drawn "
    "0.92-0.99x; halving counts mixed (huge 0.95x plain, 1.07x fused at "
    "imbalance 3.4; large 1.12-1.19x at 2.3, while large lost at 2.5 in the "
    "even cell), so no regime is claimed below the grad_weight wins.  The "
    "gate: imbalance >= 7.0 on huge and >= 4.3 on large, or on huge "
    "imbalance >= 2.0 with a mean of >= 128 units per tile, and in every "
    "case at least 4.5 units per workgroup of the measured grid (the "
    "smallest winning launch had 4.56).  Extrapolated, "
    "not measured: everything between the measured imbalances (False), "
    "in / out other than 1024, transposed operands inside the True regimes, "
    "launches with injection or a report, and devices whose grid differs "
    "from the measured one.  Registers (docs/ABLATION.md section 20): no "
    "plain variant uses scratch and no fused variant more than its "
    "single-launch twin (fused huge TT: 24 B/lane against 32)")
