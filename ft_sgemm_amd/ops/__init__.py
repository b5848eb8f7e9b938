"""Device ops: loads the in-tree HIP extension and exposes the kernel-id
dispatch surface (reference parity: sgemm.cu:110-199).

On a GPU box a missing/unbuilt extension is a hard error (no silent eager
fallback); on CPU-only hosts the golden model in .golden is the reference
implementation and the extension is not required.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from ..kernel_table import (ERR_BOUND, ERROR_INJECT, KERNEL_TABLE, TIERS)
from . import golden  # noqa: F401
from .fault_report import (BatchedFaultReport, FaultCounts,  # noqa: F401
                           FaultEvent, FaultReport, InjectionModel,
                           predict_injected_events,
                           predict_injected_events_grouped,
                           predict_injection_model)
from .grouped_streamk import (GROUPED_STREAMK_NOTE,  # noqa: F401
                              grouped_streamk_gate, grouped_streamk_layout,
                              grouped_streamk_partition,
                              grouped_streamk_units)
from .ragged_streamk import (RAGGED_STREAMK_NOTE,  # noqa: F401
                             ragged_streamk_gate, ragged_streamk_layout,
                             ragged_streamk_partition,
                             streamk_partials_floats)

_C = None
_load_err = None
try:
    from .. import _C as _C  # type: ignore
except ImportError as e:  # extension not built
    _load_err = e


def have_extension() -> bool:
    return _C is not None


def _require_ext():
    if _C is None:
        raise RuntimeError(
            "ft_sgemm_amd._C HIP extension is not built. Run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            f"(import error: {_load_err})")
    return _C


def tier_index(tier: str) -> int:
    return TIERS.index(tier)


def _launch(entry: str, tier: str, a, b, c, alpha, beta, fused=None,
            report=None, **kw):
    """The one call into the binding `entry` (sgemm, sgemm_batched or
    sgemm_ragged): plain when fused is None, otherwise the fused-ABFT twin
    with fused = (inject, tau, inj_mag, verify_windows) and the optional
    fault report.  kw: the entry's own keywords (sgemm_ragged's trans_a,
    trans_b)."""
    abft = fused is not None
    inject, tau, inj_mag, verify_windows = fused if abft else (False, 0.0,
                                                               0.0, 20)
    log = (None, None) if report is None else (report.counters, report.events)
    getattr(_require_ext(), entry)(tier_index(tier), abft, inject, a, b, c,
                                   alpha, beta, tau, inj_mag, verify_windows,
                                   *log, **kw)
    return c


def sgemm(tier: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
          alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
    """Plain hand-tiled MFMA SGEMM.  a:(K,M) b:(K,N) c:(N,M) fp32 CUDA
    tensors holding column-major A (MxK), B (NxK), C (MxN).  In-place on c."""
    return _launch("sgemm", tier, a, b, c, alpha, beta)


def ft_sgemm(tier: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
             alpha: float = 1.0, beta: float = 0.0, inject: bool = True,
             tau: float = ERR_BOUND, inj_mag: float = ERROR_INJECT,
             verify_windows: int = 20,
             report: FaultReport | None = None) -> torch.Tensor:
    """Fused-ABFT MFMA SGEMM with in-kernel verify/locate/correct.  The
    default inject=True preserves the reference's always-self-testing
    property.

    report: a FaultReport on the operands' device.  The kernel adds every
    fault it detects to it (tripped / corrected / uncorrected / unlocated
    counts and one event per fault); nothing is zeroed, so a report
    accumulates across launches until report.reset().  The launch does not
    synchronise; report.read() does.  C is bit-identical with and without
    a report."""
    return _launch("sgemm", tier, a, b, c, alpha, beta,
                   (inject, tau, inj_mag, verify_windows), report)


MAX_BATCH = 65535  # the batch index rides in gridDim.z


def batched_layout(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor):
    """Validate the operands of a strided-batched call and return
    (batch, m, n, k, sA, sB, sC), the batch strides in floats.  Runs on any
    device: the CPU-runnable mirror of the launch rules, which the C++ side
    states once, in gemm_args_error (csrc/dispatch.hip).

    a is (B, K, M) or (K, M), b is (B, K, N) or (K, N), c is (B, N, M).  A
    2-D operand is shared by every entry (stride 0), exactly like an
    expand()ed one.  The two inner dimensions must be contiguous; the batch
    stride is whatever the tensor has, so padded and expand()ed views pass
    without a copy.  Every stride must be a multiple of 4 floats and every
    tensor 16-byte aligned (16-B staging loads, f32x4 epilogue); c's entries
    must not overlap (stride >= M*N).  Raises ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_batched: {msg}")

    if c.dim() != 3:
        err(f"c must be (B, N, M), got {tuple(c.shape)}")
    batch, n, m = c.shape
    if not 1 <= batch <= MAX_BATCH:
        err(f"batch {batch} outside 1..{MAX_BATCH}")
    strides = []
    for name, x in (("a", a), ("b", b)):
        if x.dim() not in (2, 3):
            err(f"{name} must be 2-D or 3-D, got {tuple(x.shape)}")
        if x.dim() == 3 and x.shape[0] != batch:
            err(f"batch mismatch: {name} has {x.shape[0]} entries, c {batch}")
    k = a.shape[-2]
    if a.shape[-1] != m or tuple(b.shape[-2:]) != (k, n):
        err(f"a (.., K, M) = {tuple(a.shape)}, b (.., K, N) = "
            f"{tuple(b.shape)} and c (B, N, M) = {tuple(c.shape)} disagree")
    if min(m, n, k) < 1:
        err("empty matrix")
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.dtype != torch.float32:
            err(f"{name} must be float32")
        if x.stride(-1) != 1 or x.stride(-2) != x.shape[-1]:
            err(f"the two inner dimensions of {name} must be contiguous "
                f"(strides {tuple(x.stride())})")
        if x.data_ptr() % 16:
            err(f"{name} must be 16-byte aligned")
        strides.append(x.stride(0) if x.dim() == 3 and batch > 1 else 0)
    sa, sb, sc = strides
    if batch == 1:
        sc = m * n  # a single entry: the strides are not used
    if sa < 0 or sb < 0 or sa % 4 or sb % 4 or sc % 4:
        err(f"batch strides ({sa}, {sb}, {sc}) must be multiples of 4 floats")
    if sc < m * n:
        err(f"c entries overlap or are broadcast (batch stride {sc} < "
            f"M*N = {m * n})")
    return batch, m, n, k, sa, sb, sc


def _batched_operands(a, b, c):
    """(a, b) as the 3-D views the binding takes, after batched_layout."""
    batch = batched_layout(a, b, c)[0]
    return tuple(x if x.dim() == 3 else x.unsqueeze(0).expand(batch, -1, -1)
                 for x in (a, b))


def sgemm_batched(tier: str, a: torch.Tensor, b: torch.Tensor,
                  c: torch.Tensor, alpha: float = 1.0,
                  beta: float = 0.0) -> torch.Tensor:
    """Strided-batched plain SGEMM, one launch: for every entry i,
    c[i] = alpha * A_i B_i^T + beta * c[i] in sgemm's storage convention.
    a:(B,K,M) b:(B,K,N) c:(B,N,M), layout rules in batched_layout; a 2-D a
    or b is shared by all entries.  Each entry's result has the bits of
    sgemm on that entry with the classic (non-stream-K) decomposition;
    FT_SGEMM_STREAMK has no effect on a batch of more than one."""
    a3, b3 = _batched_operands(a, b, c)
    return _launch("sgemm_batched", tier, a3, b3, c, alpha, beta)


def ft_sgemm_batched(tier: str, a: torch.Tensor, b: torch.Tensor,
                     c: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
                     inject: bool = True, tau: float = ERR_BOUND,
                     inj_mag: float = ERROR_INJECT, verify_windows: int = 20,
                     report: BatchedFaultReport | None = None
                     ) -> torch.Tensor:
    """Strided-batched fused-ABFT SGEMM, one checksum-encode launch and one
    GEMM launch for the whole batch; arguments as ft_sgemm, layout as
    sgemm_batched.  A shared a (2-D or expand()ed) is encoded once.  The
    injector rotates per entry, as in ft_sgemm.  report: a
    BatchedFaultReport of the same batch size; entry i logs into slot i."""
    a3, b3 = _batched_operands(a, b, c)
    if report is not None and report.batch != c.shape[0]:
        raise ValueError(f"ft_sgemm_batched: report holds {report.batch} "
                         f"entries, the batch {c.shape[0]}")
    return _launch("sgemm_batched", tier, a3, b3, c, alpha, beta,
                   (inject, tau, inj_mag, verify_windows), report)


def ragged_layout(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                  trans_a: bool = False, trans_b: bool = False):
    """Validate the operands of a ragged call and return
    (m, n, k, lda, ldb, ldc), the leading dimensions in floats.  Runs on any
    device: the CPU-runnable mirror of the launch rules, which the C++ side
    states once, in gemm_args_error (csrc/dispatch.hip).

    a is (K, M), b is (K, N), c is (N, M), fp32, any sizes >= 1.  With
    trans_a, a is given transposed, as (M, K); with trans_b, b is (N, K).
    The inner stride must be 1 and the row stride at least the row width, so
    packed tensors and row-strided views (x[r0:r1, c0:c1]) pass without a
    copy; the row stride is the leading dimension, and a one-row tensor's is
    its width.  No alignment beyond fp32 is asked for.  c's rows must not
    overlap.  Raises ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_ragged: {msg}")

    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.dim() != 2:
            err(f"{name} must be 2-D, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            err(f"{name} must be float32")
    m, k = a.shape if trans_a else a.shape[::-1]
    n, kb = b.shape if trans_b else b.shape[::-1]
    if kb != k or tuple(c.shape) != (n, m):
        err(f"a {'(M, K)' if trans_a else '(K, M)'} = {tuple(a.shape)}, "
            f"b {'(N, K)' if trans_b else '(K, N)'} = {tuple(b.shape)} and "
            f"c (N, M) = {tuple(c.shape)} disagree")
    if min(m, n, k) < 1:
        err("empty matrix")
    lds = []
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.stride(1) != 1 and x.shape[1] != 1:
            err(f"{name} must have a unit inner stride "
                f"(strides {tuple(x.stride())})")
        if x.shape[0] == 1:
            lds.append(x.shape[1])
            continue
        if x.stride(0) < x.shape[1]:
            err(f"rows of {name} overlap or are broadcast (row stride "
                f"{x.stride(0)} < {x.shape[1]})")
        lds.append(x.stride(0))
    return (m, n, k, *lds)


def _streamk_kw(tier, layout, fused, inject, trans_a, trans_b, streamk,
                partials, device):
    """The binding keywords of a ragged call's stream-K arguments: nothing
    for streamk == 0, otherwise the clamped grid ("auto": the device grid of
    the kernel variant the call runs) and the partials buffer, allocated on
    the current stream when the caller has none."""
    if not isinstance(streamk, str) and streamk == 0:
        if partials is not None:
            raise ValueError("sgemm_ragged: partials go with streamk")
        return {}
    m, n, k = layout[:3]
    if streamk == "auto":
        ragged_streamk_layout(tier, m, n, k, 1)  # the tier has a twin
        streamk = _require_ext().ragged_streamk_grid(
            tier_index(tier), fused, inject, m, n, k, trans_a, trans_b)
        if streamk < 1:
            raise RuntimeError("sgemm_ragged: the device grid query failed")
    elif isinstance(streamk, bool) or not isinstance(streamk, int):
        raise ValueError(f"sgemm_ragged: streamk must be 0, a grid or "
                         f"'auto', got {streamk!r}")
    grid = ragged_streamk_layout(tier, m, n, k, streamk, partials)
    if partials is None:
        partials = torch.empty(streamk_partials_floats(tier, grid),
                               dtype=torch.float32, device=device)
    return dict(sk_grid=grid, partials=partials)


def sgemm_ragged(tier: str, a: torch.Tensor, b: torch.Tensor,
                 c: torch.Tensor, alpha: float = 1.0, beta: float = 0.0, *,
                 trans_a: bool = False, trans_b: bool = False,
                 streamk: int | str = 0,
                 partials: torch.Tensor | None = None) -> torch.Tensor:
    """Plain SGEMM for any M, N, K >= 1 and row-strided operands (layout
    rules in ragged_layout), on the ragged twin of `tier`'s classic kernel:
    ceil tile counts, out-of-range operand elements staged as zeros, only the
    M x N window of c written.  On a shape the tile divides the result has
    the bits of sgemm with the classic (non-stream-K) decomposition.
    In-place on c.

    trans_a / trans_b: that operand is given transposed, a as (M, K), b as
    (N, K), and read in place: c = alpha * b @ a^T + beta * c for both, the
    form of a linear layer.  The result has the bits of the untransposed
    call on x.t().contiguous().

    streamk: 0 is the classic launch, one workgroup per tile.  A positive
    int runs the stream-K decomposition on that many workgroups (tiers large
    and huge; a grid beyond the unit count is clamped), "auto" on the device
    grid, CUs x resident workgroups per CU: the work is cut into balanced
    ranges of 64-k units (ragged_streamk_partition), so a product with few
    tiles and a deep K fills the chip, and tiles that several workgroups
    share are summed in a fixed order by a second kernel.  The result is
    deterministic but, on a shared tile, not the classic launch's bits: the K
    sum is cut at other places.  ragged_streamk_gate says where it is
    expected to pay.
    partials: the buffer the shared tiles are combined through
    (ragged_streamk_layout has the rules); None allocates it with
    torch.empty on the current stream.  Neither form syncs, and with a
    caller-owned buffer a plain call can be captured in a graph."""
    layout = ragged_layout(a, b, c, trans_a, trans_b)
    return _launch("sgemm_ragged", tier, a, b, c, alpha, beta,
                   trans_a=trans_a, trans_b=trans_b,
                   **_streamk_kw(tier, layout, False, False, trans_a, trans_b,
                                 streamk, partials, c.device))


def ft_sgemm_ragged(tier: str, a: torch.Tensor, b: torch.Tensor,
                    c: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
                    inject: bool = True, tau: float = ERR_BOUND,
                    inj_mag: float = ERROR_INJECT, verify_windows: int = 20,
                    report: FaultReport | None = None, *,
                    trans_a: bool = False, trans_b: bool = False,
                    streamk: int | str = 0,
                    partials: torch.Tensor | None = None) -> torch.Tensor:
    """Fused-ABFT SGEMM for any M, N, K >= 1 and row-strided operands:
    ft_sgemm's in-kernel verify / locate / correct, injector self-test and
    fault report without a tile fit; arguments as ft_sgemm, layout and
    trans_a / trans_b as sgemm_ragged.  The injector keeps its per-block
    rule, so in an edge tile a victim may lie in the padding: it is corrected
    like any other and reported with its padded coordinates (FaultReport).
    Transposition moves no fault.

    streamk / partials: as sgemm_ragged.  Every segment of the stream-K walk
    is verified and corrected before it leaves the registers; the injector
    then fires once per (tile, group of verify_windows-derived units) of
    every segment (predict_injected_events(..., streamk_grid=)), and
    attaching a report changes neither the grid nor C."""
    layout = ragged_layout(a, b, c, trans_a, trans_b)
    return _launch("sgemm_ragged", tier, a, b, c, alpha, beta,
                   (inject, tau, inj_mag, verify_windows), report,
                   trans_a=trans_a, trans_b=trans_b,
                   **_streamk_kw(tier, layout, True, inject, trans_a, trans_b,
                                 streamk, partials, c.device))


def ragged_batched_layout(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                          trans_a: bool = False, trans_b: bool = False):
    """Validate the operands of a strided-batched ragged call and return
    (batch, m, n, k, lda, ldb, ldc, sA, sB, sC), leading dimensions and batch
    strides in floats.  Runs on any device: the CPU-runnable mirror of the
    launch rules, which the C++ side states once, in gemm_args_error
    (csrc/dispatch.hip).

    a is (B, K, M), or (B, M, K) with trans_a; b is (B, K, N), or (B, N, K)
    with trans_b; c is (B, N, M); fp32, any sizes >= 1.  A 2-D a or b is
    shared by every entry (batch stride 0), exactly like an expand()ed one.
    Per entry the rules are ragged_layout's: unit inner stride, a row stride
    of at least the row width, which is the leading dimension.  The batch
    stride is whatever the tensor has, odd ones included, and no alignment
    beyond fp32 is asked for.  c's entries must not overlap: they are either
    disjoint (sC >= (N-1)*ldc + M) or interleaved within a row (sC >= M and
    (B-1)*sC + M <= ldc), the layout of heads inside a (tokens, heads*dim)
    tensor.  Raises ValueError."""
    def err(msg):
        raise ValueError(f"sgemm_ragged_batched: {msg}")

    if c.dim() != 3:
        err(f"c must be (B, N, M), got {tuple(c.shape)}")
    batch, n, m = c.shape
    for name, x in (("a", a), ("b", b)):
        if x.dim() not in (2, 3):
            err(f"{name} must be 2-D or 3-D, got {tuple(x.shape)}")
        if x.dim() == 3 and x.shape[0] != batch:
            err(f"batch mismatch: {name} has {x.shape[0]} entries, c {batch}")
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.dtype != torch.float32:
            err(f"{name} must be float32")
    ma, k = a.shape[-2:] if trans_a else a.shape[-2:][::-1]
    nb, kb = b.shape[-2:] if trans_b else b.shape[-2:][::-1]
    if (ma, nb, kb) != (m, n, k):
        err(f"a {'(.., M, K)' if trans_a else '(.., K, M)'} = "
            f"{tuple(a.shape)}, b {'(.., N, K)' if trans_b else '(.., K, N)'} "
            f"= {tuple(b.shape)} and c (B, N, M) = {tuple(c.shape)} disagree")
    if min(batch, m, n, k) < 1:
        err("empty batch or matrix")
    if batch > MAX_BATCH:
        err(f"batch {batch} outside 1..{MAX_BATCH}")
    lds, strides = [], []
    for name, x in (("a", a), ("b", b), ("c", c)):
        if x.stride(-1) != 1 and x.shape[-1] != 1:
            err(f"{name} must have a unit inner stride "
                f"(strides {tuple(x.stride())})")
        if x.shape[-2] == 1:
            lds.append(x.shape[-1])
        elif x.stride(-2) < x.shape[-1]:
            err(f"rows of {name} overlap or are broadcast (row stride "
                f"{x.stride(-2)} < {x.shape[-1]})")
        else:
            lds.append(x.stride(-2))
        strides.append(x.stride(0) if x.dim() == 3 and batch > 1 else 0)
    lda, ldb, ldc = lds
    sa, sb, sc = strides
    if batch > 1:
        if sc == 0:
            err("c is broadcast over the batch (batch stride 0)")
        disjoint = sc >= (n - 1) * ldc + m
        interleaved = sc >= m and (batch - 1) * sc + m <= ldc
        if not (disjoint or interleaved):
            err(f"c entries overlap (batch stride {sc}, row stride {ldc}, "
                f"N = {n}, M = {m})")
    return batch, m, n, k, lda, ldb, ldc, sa, sb, sc


def _ragged_batched_operands(a, b, c, trans_a, trans_b):
    """(a, b) as the 3-D views the binding takes, after
    ragged_batched_layout."""
    batch = ragged_batched_layout(a, b, c, trans_a, trans_b)[0]
    return tuple(x if x.dim() == 3 else x.unsqueeze(0).expand(batch, -1, -1)
                 for x in (a, b))


def sgemm_ragged_batched(tier: str, a: torch.Tensor, b: torch.Tensor,
                         c: torch.Tensor, alpha: float = 1.0,
                         beta: float = 0.0, *, trans_a: bool = False,
                         trans_b: bool = False) -> torch.Tensor:
    """Strided-batched plain SGEMM for any M, N, K >= 1, one launch: for
    every entry i, c[i] = alpha * A_i B_i^T + beta * c[i] in sgemm_ragged's
    conventions, trans_a / trans_b included.  Layout rules in
    ragged_batched_layout; a 2-D a or b is shared by all entries.  c[i] has
    the bits of sgemm_ragged on the views a[i], b[i], c[i].  In-place on c."""
    a3, b3 = _ragged_batched_operands(a, b, c, trans_a, trans_b)
    return _launch("sgemm_ragged_batched", tier, a3, b3, c, alpha, beta,
                   trans_a=trans_a, trans_b=trans_b)


def ft_sgemm_ragged_batched(tier: str, a: torch.Tensor, b: torch.Tensor,
                            c: torch.Tensor, alpha: float = 1.0,
                            beta: float = 0.0, inject: bool = True,
                            tau: float = ERR_BOUND,
                            inj_mag: float = ERROR_INJECT,
                            verify_windows: int = 20,
                            report: BatchedFaultReport | None = None, *,
                            trans_a: bool = False, trans_b: bool = False
                            ) -> torch.Tensor:
    """Strided-batched fused-ABFT SGEMM for any M, N, K >= 1: one
    checksum-encode launch and one GEMM launch for the whole batch; arguments
    as ft_sgemm_ragged, layout as sgemm_ragged_batched.  A shared a (2-D or
    expand()ed) is encoded once.  The injector keeps its per-block rule in
    every entry, so a victim may lie in an edge tile's padding and is then
    reported with its padded coordinates.  report: a BatchedFaultReport of
    the same batch size; entry i logs into slot i."""
    a3, b3 = _ragged_batched_operands(a, b, c, trans_a, trans_b)
    if report is not None and report.batch != c.shape[0]:
        raise ValueError(f"ft_sgemm_ragged_batched: report holds "
                         f"{report.batch} entries, the batch {c.shape[0]}")
    return _launch("sgemm_ragged_batched", tier, a3, b3, c, alpha, beta,
                   (inject, tau, inj_mag, verify_windows), report,
                   trans_a=trans_a, trans_b=trans_b)


def rocblas_sgemm(a, b, c, alpha: float = 1.0, beta: float = 0.0):
    """Kernel id 0: the vendor-BLAS oracle."""
    _require_ext().rocblas_sgemm(a, b, c, alpha, beta)
    return c


def baseline_ft(a, b, c, alpha: float = 1.0, beta: float = 0.0,
                panel_k: int = 1024, fault=None, per_panel: bool = False):
    """Kernel id 10: non-fused rocBLAS ABFT chain.  Returns (c, (res_row,
    res_col)): the squared residual norms of the worst verified panel, NaN
    or Inf whenever any panel's was.

    fault: test seam, (panel, i, j, value, overwrite) — after the GEMM of
    K panel `panel` the element (i, j) of the M x N result (c[j, i]) gets
    += value, or = value when overwrite.  Out-of-range indices raise before
    anything is launched.
    per_panel: also return every verdict computed, in order, as a third
    item [(panel, res_row, res_col), ...]."""
    if fault is not None:
        p, i, j, value, overwrite = fault
        fault = (int(p), int(i), int(j), float(value), bool(overwrite))
    res_row, res_col, panels = _require_ext().baseline_ft(
        a, b, c, alpha, beta, panel_k, fault)
    if per_panel:
        return c, (res_row, res_col), panels
    return c, (res_row, res_col)


def selftest_descriptors(rows):
    """Pack self-test cases into the (idesc, fdesc) arrays the three
    self-test entries take.  rows: a list of (faults, tau), faults a list of
    at most two (fm, fn, reg, lane, mag).  Returns CPU numpy arrays: idesc
    (ncases, 9) int32 = {nfault, (fm, fn, reg, lane) x 2} and fdesc
    (ncases, 3) float32 = {mag0, mag1, tau}, unused slots zero."""
    idesc = np.zeros((len(rows), 9), dtype=np.int32)
    fdesc = np.zeros((len(rows), 3), dtype=np.float32)
    for i, (faults, tau) in enumerate(rows):
        if len(faults) > 2:
            raise ValueError(f"case {i}: {len(faults)} faults, at most 2")
        idesc[i, 0] = len(faults)
        for f, (fm, fn, reg, lane, mag) in enumerate(faults):
            idesc[i, 1 + 4 * f:5 + 4 * f] = (fm, fn, reg, lane)
            fdesc[i, f] = mag
        fdesc[i, 2] = tau
    return idesc, fdesc


def locate_selftest_report(fm: int, fn: int, mm: int, idesc: torch.Tensor,
                           fdesc: torch.Tensor, amp: float,
                           capacity: int = 4):
    """locate_selftest's report twin: runs only the shipped locate/correct,
    with a fault log per case (wave tile at origin (0, 0), k range [0, 0)),
    on the same descriptors.  Returns (tiles (ncases, fm*fn*nreg, 64),
    counters (ncases, 5) int32, events (ncases, capacity, 8) int32);
    fault_report.decode(counters[c], events[c]) decodes one case."""
    return _require_ext().locate_selftest_report(fm, fn, mm, idesc, fdesc,
                                                 amp, capacity)


def locate_selftest(fm: int, fn: int, mm: int, idesc: torch.Tensor,
                    fdesc: torch.Tensor, amp: float) -> torch.Tensor:
    """Device self-test of the fused kernels' locate/correct on a synthetic
    fm x fn wave tile of mm-wide MFMA fragments, one single-wave block per
    case.  idesc (ncases, 9) int32 = {nfault, (fm, fn, reg, lane) x 2},
    fdesc (ncases, 3) fp32 = {mag0, mag1, tau}; clean accumulators are a
    hash in (-amp, amp).  Returns (3, ncases, fm*fn*nreg, 64): the tile
    corrected by the shipped function, by the sweep-everything reference
    form, and the clean tile."""
    return _require_ext().locate_selftest(fm, fn, mm, idesc, fdesc, amp)


def detect_selftest(fm: int, fn: int, mm: int, idesc: torch.Tensor,
                    fdesc: torch.Tensor, amp: float) -> torch.Tensor:
    """locate_selftest's detect twin: runs only the fused kernels' shared
    detect and the locate's fp32 screen on the same descriptors and the same
    synthetic tile.  Returns (ncases, fm*fn*nreg + 1 + 2*fn, 64), lane last:
    rows [0, fm*fn*nreg) the faulty tile (element (fm*FN + fn)*nreg + reg),
    then the wave residual the detect compares with tau (the same in all 64
    lanes), then per fn the lane's partial sum p[fn] over fm and reg, then
    per fn 1.0 where the screen passed the fragment column and 0.0 where it
    did not."""
    return _require_ext().detect_selftest(fm, fn, mm, idesc, fdesc, amp)


def choose_tier(m: int, n: int, k: int, batch: int = 1,
                ragged: bool = False):
    """Pick the fastest applicable tier for a problem shape, or None when no
    hand-tiled tier divides the shape (callers fall back to rocBLAS).

    Thresholds from the final measured 1024..6144 sweep
    (profiles/cli_sweep_r2.log, stream-K-enabled kernels): the huge
    256x128 macro-tile wins from ~384 tiles up (its stream-K twin covers
    the tail-waste sizes), the large 64x64 tier wins the 2048-3072 band
    (>=1024 blocks), and below that the medium tier's dense grid wins.

    batch: entries of a strided-batched launch (sgemm_batched /
    ft_sgemm_batched).  batch == 1 gives exactly the single-launch answers
    above.  For batch > 1 the same thresholds are applied to the grid the
    launch really has, tiles x batch workgroups: in the four measured cells
    of profiles/batched_bmm.txt (512^3 x64, 1024^3 x16, 2048^3 x4 -> huge;
    block_row panel 1024x1024x512 x8 -> large) that picks the fastest tier.
    BATCHED_THRESHOLDS_NOTE has the details and what is not measured.

    ragged: pick for sgemm_ragged / ft_sgemm_ragged.  Every tier then fits
    every shape, so a tier is always returned: the same thresholds, applied
    to the ceil tile counts of the grid the ragged launch has.  Where the
    plain call returns a tier, this returns the same one.
    RAGGED_THRESHOLDS_NOTE says what of this is measured."""
    from .. import kernel_table as kt

    def fits(tier):
        t = kt.TILING[tier]
        return ragged or (m % t["bm"] == 0 and n % t["bn"] == 0 and
                          k % t["bk"] == 0)

    def tiles(tier):
        t = kt.TILING[tier]
        return -(-m // t["bm"]) * -(-n // t["bn"])

    if ragged:
        if batch != 1 or min(m, n, k) < 1:
            raise ValueError("choose_tier: a ragged launch is one product "
                             "of sizes >= 1")
        # a shape some tier divides keeps the tier its tiled launch gets
        tiled = choose_tier(m, n, k)
        if tiled is not None:
            return tiled
    if fits("huge") and tiles("huge") * batch >= 384:
        return "huge"
    skinny = ("tall" if m >= 4 * n else "wide" if n >= 4 * m else None)
    if skinny and fits(skinny):
        return skinny
    if fits("large") and tiles("large") * batch >= 1024:
        return "large"
    for tier in ("medium", "large", "small"):
        if fits(tier):
            return tier
    return None


# How choose_tier's batch > 1 answers were arrived at.
BATCHED_THRESHOLDS_NOTE = (
    "measured (profiles/batched_bmm.txt, MI355X, one batched launch, plain "
    "and fused no-inject): the single-launch tile-count thresholds applied "
    "to tiles x batch pick the fastest measured tier in all four cells — "
    "512^3 x64, 1024^3 x16 and 2048^3 x4 (each 512 huge tiles x batch: huge "
    "is 16-22% ahead of the next tier) and the block_row panel 1024x1024x512 "
    "x8 (256 huge tiles x batch, below 384: large, 1-2% ahead of huge).  "
    "Grids between 256 and 512 huge tiles and skinny batched shapes are "
    "not measured")


# How choose_tier's ragged=True answers were arrived at.
RAGGED_THRESHOLDS_NOTE = (
    "a shape some tier divides keeps the tier of its tiled launch; any other "
    "shape gets the single-launch tile-count thresholds applied to ceil tile "
    "counts.  The thresholds are inherited, not fitted to ragged runs.  "
    "measured (profiles/ragged.txt, MI355X, plain and fused no-inject), six "
    "cells: 5001^3 (800 huge tiles) and 6145^3 (1225) -> huge, which is "
    "6-20% ahead of large; 4097^3 and 4100^3 (561 huge tiles: a full round of 512 "
    "resident workgroups plus a tail round of 49) -> huge, but large is "
    "5-19% FASTER there: the ragged path has no stream-K to absorb the tail "
    "round; skinny 8193x257x1025 -> tall, but medium is 24% faster (large "
    "4-15%); small 1000x1000x333 -> medium, level with small plain and 9% "
    "behind it fused, 29-41% ahead of large.  The choice is left as "
    "specified; correcting the two losing cells needs a tail-round rule and "
    "a skinny sweep that two shapes do not support.  Every other shape is "
    "not measured")


def choose_tier_ragged_batched(m: int, n: int, k: int, batch: int) -> str:
    """Pick the tier for sgemm_ragged_batched / ft_sgemm_ragged_batched.
    Every tier fits every shape, so a tier is always returned: choose_tier's
    batched rule on the grid the ragged launch has, i.e. the single-launch
    tile-count thresholds applied to ceil tile counts x batch workgroups.
    batch == 1 gives choose_tier(m, n, k, ragged=True); a shape some tier
    divides keeps the tier choose_tier(m, n, k, batch) gives its tiled batch.
    RAGGED_BATCHED_THRESHOLDS_NOTE says what of this is measured."""
    from .. import kernel_table as kt

    if min(m, n, k, batch) < 1:
        raise ValueError("choose_tier_ragged_batched: sizes and batch must "
                         "be >= 1")
    tiled = choose_tier(m, n, k, batch)
    if tiled is not None:
        return tiled

    def tiles(tier):
        t = kt.TILING[tier]
        return -(-m // t["bm"]) * -(-n // t["bn"])

    if tiles("huge") * batch >= 384:
        return "huge"
    if m >= 4 * n:
        return "tall"
    if n >= 4 * m:
        return "wide"
    if tiles("large") * batch >= 1024:
        return "large"
    return "medium"


# How choose_tier_ragged_batched's answers were arrived at.
RAGGED_BATCHED_THRESHOLDS_NOTE = (
    "the single-launch tile-count thresholds applied to ceil tile counts x "
    "batch, with a shape some tier divides keeping the tier of its tiled "
    "batch.  The thresholds are inherited, not fitted to ragged batched "
    "runs.  measured (profiles/ragged_batched.txt, MI355X, one batched "
    "launch, plain and fused no-inject, the chosen tier against huge, large "
    "and medium), four cells: 1024^3 x16 aligned -> huge, 20-26% ahead of "
    "large; attention scores 1000x1000x80 x32 NT (32 huge tiles x 32) -> "
    "huge, which is 5% ahead of large fused and 5% BEHIND it plain; "
    "attention context 80x1000x1000 x32 NT (skinny, 256 huge tiles) -> wide, "
    "but medium is 23% (plain) and 35% (fused) FASTER; 1025^3 x16 (45 huge "
    "tiles x 16, 13 of each 45 edge tiles with one real row or column) -> "
    "huge, but large is 27% "
    "(plain) and 21% (fused) FASTER.  The choice is left as specified: two "
    "losing cells do not support a rule for edge-tile waste or for skinny "
    "batches.  Every other shape is not measured")


def sgemm_auto(a, b, c, alpha: float = 1.0, beta: float = 0.0):
    """Plain SGEMM with automatic tier selection; shapes no hand-written
    tier divides (e.g. M=100) fall back to the rocBLAS vendor path instead
    of raising."""
    k, m = a.shape
    n = b.shape[1]
    tier = choose_tier(m, n, k)
    if tier is None:
        return rocblas_sgemm(a, b, c, alpha, beta)
    return sgemm(tier, a, b, c, alpha, beta)


def ft_sgemm_auto(a, b, c, alpha: float = 1.0, beta: float = 0.0,
                  inject: bool = True, report: FaultReport | None = None,
                  misfit: str = "baseline"):
    """Fused-ABFT SGEMM with automatic tier selection.  What happens to a
    shape no tier divides is the caller's choice:

    misfit="baseline" (the default): the rocBLAS GEMM wrapped in the OFFLINE
    checksum ABFT chain (kernel id 10 semantics: detection verdicts, no
    in-kernel correction); a verdict above the threshold of ERR_BOUND^2, or
    one that is NaN or Inf, raises, making silent corruption impossible on
    the fallback path.
    misfit="ragged": ft_sgemm_ragged on choose_tier(..., ragged=True) — the
    fused kernel's in-register locate/correct, injector self-test and fault
    report, for any shape.

    report: passed to ft_sgemm when a tier fits, and to ft_sgemm_ragged.  On
    the rocBLAS fallback branch the report is left untouched: that branch
    has no in-kernel locate/correct to report on, and it already raises on
    a tripped verdict."""
    if misfit not in ("baseline", "ragged"):
        raise ValueError(f"ft_sgemm_auto: misfit must be 'baseline' or "
                         f"'ragged', got {misfit!r}")
    k, m = a.shape
    n = b.shape[1]
    tier = choose_tier(m, n, k)
    if tier is None and misfit == "ragged":
        return ft_sgemm_ragged(choose_tier(m, n, k, ragged=True), a, b, c,
                               alpha, beta, inject=inject, report=report)
    if tier is None:
        pk = k if k <= 1024 or k % 1024 else 1024
        _, (res_row, res_col) = baseline_ft(a, b, c, alpha, beta, panel_k=pk)
        # Squared residual l2 norms; fault-free roundoff at these operand
        # scales is orders of magnitude below ERR_BOUND^2.  Clean means
        # both finite and within it: a NaN verdict (a NaN left in C) fails
        # every comparison, so the test is for clean, not for tripped.
        limit = ERR_BOUND * ERR_BOUND
        if not (math.isfinite(res_row) and math.isfinite(res_col) and
                res_row <= limit and res_col <= limit):
            raise RuntimeError(
                f"ft_sgemm_auto fallback: offline ABFT verdict tripped "
                f"(res_row={res_row:.3e}, res_col={res_col:.3e}) — "
                f"uncorrectable fault in the rocBLAS fallback GEMM")
        return c
    return ft_sgemm(tier, a, b, c, alpha, beta, inject=inject, report=report)


def run_kernel_id(kid: int, a, b, c, alpha: float = 1.0, beta: float = 0.0,
                  inject: bool = True, report: FaultReport | None = None):
    """Dispatch by reference kernel id (0=rocBLAS, 1-6 plain tiers,
    7-9 rocBLAS fallback, 10 baseline, 11-16 fused-ABFT tiers).  `report`
    is accepted for the fused ids only."""
    if report is not None and not (kid in KERNEL_TABLE and
                                   KERNEL_TABLE[kid][2]):
        raise ValueError(f"kernel id {kid} has no fault report "
                         f"(fused-ABFT ids 11-16 only)")
    if kid in (0, 7, 8, 9):
        return rocblas_sgemm(a, b, c, alpha, beta)
    if kid == 10:
        return baseline_ft(a, b, c, alpha, beta)[0]
    name, tier, fused = KERNEL_TABLE[kid]
    if fused:
        return ft_sgemm(tier, a, b, c, alpha, beta, inject=inject,
                        report=report)
    return sgemm(tier, a, b, c, alpha, beta)


def make_operands(m: int, n: int, k: int, device="cuda", seed: int = 10):
    """Column-major operands as (K,M)/(K,N)/(N,M) contiguous tensors with
    the reference value distribution (uniform (-0.9, 0.9), utils.cu:23)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.rand((k, m), generator=g) * 1.8 - 0.9).to(device)
    b = (torch.rand((k, n), generator=g) * 1.8 - 0.9).to(device)
    c = torch.zeros((n, m), device=device)
    return a, b, c


def torch_reference(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                    alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
    """Plain fp32 PyTorch reference of the same op: c' = alpha*(b^T a) + beta*c
    (in our storage convention this IS C = alpha*A B^T + beta*C)."""
    return alpha * (b.transpose(0, 1) @ a) + beta * c


def torch_reference_batched(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
                            alpha: float = 1.0,
                            beta: float = 0.0) -> torch.Tensor:
    """torch.bmm form of torch_reference for a:(B,K,M) b:(B,K,N) c:(B,N,M);
    a 2-D a or b is shared by all entries."""
    batch = c.shape[0]
    a3, b3 = (x if x.dim() == 3 else x.unsqueeze(0).expand(batch, -1, -1)
              for x in (a, b))
    return alpha * torch.bmm(b3.transpose(1, 2), a3) + beta * c


from .linear import FTLinear, ft_linear  # noqa: E402,F401
from .bmm import ft_bmm  # noqa: E402,F401
from .grouped import (GROUPED_THRESHOLDS_NOTE, GroupedPlan,  # noqa: E402,F401
                      choose_tier_grouped, ft_sgemm_grouped, grouped_layout,
                      sgemm_grouped)
from .grouped_linear import ft_grouped_linear  # noqa: E402,F401
