"""Grouped ragged SGEMM: one launch for a list of products, each with its own
M, N, K, leading dimensions and pointers (csrc/ft_ragged.hpp, GROUPED).

The strided-batched calls need one shape and one stride for the whole batch;
a grouped call takes sequences of 2-D tensors instead.  A one-dimensional
grid covers the tiles of all entries, and a descriptor table on the device
(csrc/grouped_table.h) tells each block which entry it belongs to.  Entry e
has the bits of ops.sgemm_ragged / ops.ft_sgemm_ragged on its own operands.
"""

from __future__ import annotations

import torch

from ..kernel_table import ERR_BOUND, ERROR_INJECT
from .fault_report import BatchedFaultReport

MAX_GROUPED_TILES = 2 ** 31 - 1  # the tile index rides in gridDim.x


def _entry_layout(e, a, b, c, trans_a, trans_b, err):
    """ragged_layout's per-entry rules with empty sizes allowed."""
    for name, x in (("a", a), ("b", b), ("c", c)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            err(f"entry {e}: {name} must be a 2-D tensor")
        if x.dtype != torch.float32:
            err(f"entry {e}: {name} must be float32")
    m, k = a.shape if trans_a else a.shape[::-1]
    n, kb = b.shape if trans_b else b.shape[::-1]
    if kb != k or tuple(c.shape) != (n, m):
        err(f"entry {e}: a {'(M, K)' if trans_a else '(K, M)'} = "
            f"{tuple(a.shape)}, b {'(N, K)' if trans_b else '(K, N)'} = "
            f"{tuple(b.shape)} and c (N, M) = {tuple(c.shape)} disagree")
    lds = []
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.numel() == 0:  # never read or written: any strides
            lds.append(max(x.shape[1], 1))
            continue
        if x.stride(1) != 1 and x.shape[1] != 1:
            err(f"entry {e}: {name} must have a unit inner stride "
                f"(strides {tuple(x.stride())})")
        if x.shape[0] == 1:
            lds.append(x.shape[1])
            continue
        if x.stride(0) < x.shape[1]:
            err(f"entry {e}: rows of {name} overlap or are broadcast (row "
                f"stride {x.stride(0)} < {x.shape[1]})")
        lds.append(x.stride(0))
    return (m, n, k, *lds)


def grouped_layout(a_list, b_list, c_list, trans_a: bool = False,
                   trans_b: bool = False):
    """Validate the operands of a grouped call and return the list of
    per-entry (m, n, k, lda, ldb, ldc).  Runs on any device: the CPU-runnable
    mirror of the launch rules, which the C++ side states once, in
    grouped_args_error (csrc/dispatch.hip).

    a_list, b_list and c_list are sequences of the same length >= 1.  Entry e
    follows ragged_layout: a (K, M), or (M, K) with trans_a; b (K, N), or
    (N, K) with trans_b; c (N, M); fp32, unit inner stride, rows that do not
    overlap, no alignment beyond fp32.  Unlike a single ragged call an entry
    may be empty: with M == 0 or N == 0 it has nothing to do, with K == 0 and
    M, N > 0 it computes c = beta * c.  All tensors lie on one device.

    The c entries are written, so their footprints — for a non-empty c the
    address interval from its first to its last element — must be pairwise
    disjoint.  Entries interleaved within a row of a wider tensor (the heads
    of a (tokens, heads*dim) tensor, which the strided-batched call accepts)
    have intersecting footprints and are not supported in this form.  Raises
    ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_grouped: {msg}")

    lists = [list(x) for x in (a_list, b_list, c_list)]
    if not (len(lists[0]) == len(lists[1]) == len(lists[2])):
        err(f"a_list, b_list and c_list hold {len(lists[0])}, "
            f"{len(lists[1])} and {len(lists[2])} entries")
    if not lists[2]:
        err("empty group")
    device = lists[2][0].device if isinstance(lists[2][0],
                                              torch.Tensor) else None
    out, spans, tiles = [], [], 0
    for e, (a, b, c) in enumerate(zip(*lists)):
        lay = _entry_layout(e, a, b, c, trans_a, trans_b, err)
        if not (a.device == b.device == c.device == device):
            err(f"entry {e}: all tensors must be on one device")
        m, n, _, _, _, ldc = lay
        if m and n:
            start = c.data_ptr() // 4
            spans.append((start, start + (n - 1) * ldc + m, e))
        out.append(lay)
    spans.sort()
    reach, owner = None, None
    for start, end, e in spans:
        if reach is not None and start < reach:
            err(f"c of entries {owner} and {e} overlap (their address "
                f"intervals intersect; entries interleaved within a row are "
                f"not supported by a grouped call)")
        if reach is None or end > reach:
            reach, owner = end, e
    return out


def _total_tiles(shapes, tier):
    from .. import kernel_table as kt
    t = kt.TILING[tier]
    return sum(-(-s[0] // t["bm"]) * -(-s[1] // t["bn"]) for s in shapes)


def choose_tier_grouped(shapes) -> str:
    """Pick the tier for sgemm_grouped / ft_sgemm_grouped from the per-entry
    shapes (m, n, k, ...), as grouped_layout returns them.  Every tier fits
    every entry, so a tier is always returned.  One entry with sizes >= 1
    gets choose_tier(m, n, k, ragged=True).  Otherwise the single-launch
    tile-count thresholds are applied to the grid the launch has, the ceil
    tile counts summed over the entries; the skinny tiers are taken when the
    summed M and N are 4:1 apart.  GROUPED_THRESHOLDS_NOTE says what of this
    is measured."""
    from . import choose_tier
    live = [tuple(s[:3]) for s in shapes if s[0] > 0 and s[1] > 0]
    if len(live) == 1 and live[0][2] > 0:
        return choose_tier(*live[0], ragged=True)
    if _total_tiles(live, "huge") >= 384:
        return "huge"
    m_sum, n_sum = sum(s[0] for s in live), sum(s[1] for s in live)
    if live and m_sum >= 4 * n_sum:
        return "tall"
    if live and n_sum >= 4 * m_sum:
        return "wide"
    if _total_tiles(live, "large") >= 1024:
        return "large"
    return "medium"


# How choose_tier_grouped's answers were arrived at.
GROUPED_THRESHOLDS_NOTE = (
    "the single-launch tile-count thresholds applied to the ceil tile counts "
    "summed over the entries, a single entry keeping the tier of its single "
    "ragged launch.  The thresholds are inherited, not fitted to grouped "
    "runs; the skinny rule on summed M and N is a guess in the same spirit.  "
    "profiles/grouped.txt holds what was measured (mixture-of-experts "
    "forward and backward products against the loop of single launches, the "
    "padded batched launch and torch); a cell where another tier would have "
    "won is reported there and in docs/ABLATION.md, not corrected here")


class GroupedPlan:
    """The descriptor table and the workspace of one grouped launch, built
    and uploaded once; run() then launches with no allocation, no copy and no
    sync, as often as wanted (the operands are read where they lie each
    time).  The plan keeps the tensors alive.

    tier, a_list, b_list, c_list, trans_a, trans_b: as sgemm_grouped.
    fused: plan the fused-ABFT twin; the table's verify windows depend on it
    and on verify_windows, so a plan is one or the other.
    workspace: the fused launch's segment-checksum scratch (empty for a plain
    plan); every run() rewrites all of it that is read.

    streamk: 0 (the default) plans the classic launch, one workgroup per
    output tile.  G >= 1 plans the grouped stream-K launch
    (csrc/ft_ragged_grouped_streamk.hpp) on G workgroups, "auto" on the
    device grid (CUs x resident workgroups of the kernel the plan selects):
    the 64-k units of all entries, K == 0 entries counting one empty unit
    per tile, are cut into balanced contiguous ranges, so a deep entry is
    shared by many workgroups and a shallow one costs little.  Tiers large
    and huge only.  The grid is clamped to the unit count and fixed for the
    plan (streamk_grid reports it; 0 for a classic plan or a group without
    units), since the partials buffer is sized by it.
    partials: the buffer split tiles are combined through, a contiguous
    16-byte aligned fp32 tensor of at least
    streamk_partials_floats(tier, streamk_grid) elements on the operands'
    device; None lets the plan allocate it once, here.  Nothing in it has to
    be initialised and nothing is kept in it between runs.  Tiles one
    workgroup owns whole have the classic launch's bits; split tiles are
    summed in a fixed order, so every run gives the same bits."""

    def __init__(self, tier: str, a_list, b_list, c_list, *,
                 fused: bool = False, trans_a: bool = False,
                 trans_b: bool = False, verify_windows: int = 20,
                 streamk=0, partials: torch.Tensor | None = None):
        from . import _require_ext, tier_index
        from .grouped_streamk import grouped_streamk_layout
        a_list, b_list, c_list = list(a_list), list(b_list), list(c_list)
        self.shapes = grouped_layout(a_list, b_list, c_list, trans_a, trans_b)
        self.tier, self.fused = tier, bool(fused)
        self.groups = len(c_list)
        if streamk == "auto":
            sk_grid = -1
            grouped_streamk_layout(tier, self.shapes, 1)
        elif isinstance(streamk, bool) or not isinstance(streamk, int) \
                or streamk < 0:
            raise ValueError(f"GroupedPlan: streamk must be 0, a grid >= 1 "
                             f"or 'auto', got {streamk!r}")
        else:
            sk_grid = streamk
            if sk_grid:
                grouped_streamk_layout(tier, self.shapes, sk_grid, partials)
        if not sk_grid and partials is not None:
            raise ValueError("GroupedPlan: partials go with streamk")
        self._impl = _require_ext().GroupedPlan(
            tier_index(tier), self.fused, a_list, b_list, c_list,
            bool(trans_a), bool(trans_b), int(verify_windows), sk_grid,
            partials)
        self._c = c_list

    @property
    def workspace(self) -> torch.Tensor:
        return self._impl.workspace

    @property
    def streamk_grid(self) -> int:
        return self._impl.streamk_grid

    @property
    def partials(self) -> torch.Tensor | None:
        return self._impl.partials

    def run(self, alpha: float = 1.0, beta: float = 0.0, *,
            inject: bool = False, tau: float = ERR_BOUND,
            inj_mag: float = ERROR_INJECT,
            report: BatchedFaultReport | None = None):
        """One grouped launch (fused: one encode launch before it) on the
        current stream; returns the c tensors, written in place."""
        if not self.fused and (inject or report is not None):
            raise ValueError("GroupedPlan.run: inject and report need a "
                             "fused plan")
        if report is not None and report.batch != self.groups:
            raise ValueError(f"GroupedPlan.run: report holds {report.batch} "
                             f"entries, the group {self.groups}")
        log = (None, None) if report is None else (report.counters,
                                                   report.events)
        self._impl.run(alpha, beta, inject, tau, inj_mag, *log)
        return self._c


def sgemm_grouped(tier: str, a_list, b_list, c_list, alpha: float = 1.0,
                  beta: float = 0.0, *, trans_a: bool = False,
                  trans_b: bool = False, streamk=0,
                  partials: torch.Tensor | None = None):
    """Grouped plain SGEMM, one launch: for every entry e,
    c_list[e] = alpha * A_e B_e^T + beta * c_list[e] in sgemm_ragged's
    conventions, each entry with its own sizes, leading dimensions and
    pointers (layout rules in grouped_layout).  alpha, beta and the transpose
    flags are common to the launch.  c_list[e] has the bits of sgemm_ragged
    on (a_list[e], b_list[e], c_list[e]); an entry with K == 0 becomes
    beta * c (exact zeros for beta == 0, c not read).  In place on the c
    tensors, which are returned.  Builds a GroupedPlan and runs it once.
    streamk, partials: the grouped stream-K launch, as GroupedPlan's; split
    tiles then differ from sgemm_ragged in summation order only."""
    return GroupedPlan(tier, a_list, b_list, c_list, fused=False,
                       trans_a=trans_a, trans_b=trans_b, streamk=streamk,
                       partials=partials).run(alpha, beta)


def ft_sgemm_grouped(tier: str, a_list, b_list, c_list, alpha: float = 1.0,
                     beta: float = 0.0, inject: bool = True,
                     tau: float = ERR_BOUND, inj_mag: float = ERROR_INJECT,
                     verify_windows: int = 20,
                     report: BatchedFaultReport | None = None, *,
                     trans_a: bool = False, trans_b: bool = False,
                     streamk=0, partials: torch.Tensor | None = None):
    """Grouped fused-ABFT SGEMM: one checksum-encode launch and one GEMM
    launch for all entries; arguments as ft_sgemm_ragged, operands as
    sgemm_grouped.  Every entry's A is encoded by itself into its own region
    of one workspace.  Entry e has the bits, and reports the events, of
    ft_sgemm_ragged on its own operands; an entry with K == 0 injects
    nothing.  report: a BatchedFaultReport of len(c_list) entries; entry e
    logs into slot e, an entry without tiles leaves its slot untouched.
    streamk, partials: the grouped stream-K launch, as GroupedPlan's; the
    events are then those of
    fault_report.predict_injected_events_grouped(..., streamk_grid=grid)."""
    return GroupedPlan(tier, a_list, b_list, c_list, fused=True,
                       trans_a=trans_a, trans_b=trans_b,
                       verify_windows=verify_windows, streamk=streamk,
                       partials=partials).run(
                           alpha, beta, inject=inject, tau=tau,
                           inj_mag=inj_mag, report=report)
