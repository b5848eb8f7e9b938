"""Multi-GPU scaling over RCCL/xGMI (torch.distributed, one process per GPU).

The reference is strictly single-GPU (no NCCL/MPI anywhere);
these are the new first-class components mandated by BASELINE.json:

* replicated weak scaling — one independent square SGEMM per GPU, aggregate
  GFLOPS curve over 1/2/4/8 MI355X (configs[4a]);
* block-row-distributed large-N SGEMM — A and C partitioned by block rows
  across ranks, B K-panels all-gathered with RCCL over xGMI and
  double-buffered against local fused-ABFT MFMA compute (configs[4b]).
  xGMI is 7 point-to-point links per GPU, so the all-gather of a panel
  spreads traffic over every link; panels are sized so that gather(p+1)
  overlaps compute(p) (async collectives on RCCL's internal stream).

Everything here is backend-agnostic: `gloo` + CPU matmul exercises the same
code path in CI containers without GPUs (tests/test_distributed.py).
"""

from __future__ import annotations

import os
from typing import Callable, Optional

import torch
import torch.distributed as dist


def init_from_env(backend: Optional[str] = None) -> tuple[int, int]:
    """Initialise torch.distributed from torchrun-style env vars.
    Returns (rank, world_size); world_size 1 with no env works too."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
        # one GPU per rank on the device backend only: a gloo (CPU) job may
        # run more ranks than the box has GPUs
        if backend == "nccl" and torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
    return rank, world


def local_shard(full_cols: int, rank: int, world: int) -> tuple[int, int]:
    """Even block partition [lo, hi) of a dimension across ranks."""
    assert full_cols % world == 0, (
        f"dimension {full_cols} must divide world size {world}")
    per = full_cols // world
    return rank * per, (rank + 1) * per


def replicated_weak_scaling_step(gemm_fn: Callable[[], None]) -> None:
    """One step of the replication harness: every rank runs an independent
    GEMM; synchronisation is done by the caller's timing bracket."""
    gemm_fn()


def block_row_sgemm(a_local: torch.Tensor, b_local: torch.Tensor,
                    c_local: torch.Tensor, *, panel_k: int,
                    gemm_fn: Callable[..., None], alpha: float = 1.0,
                    beta: float = 0.0,
                    group: Optional[dist.ProcessGroup] = None,
                    batched_gemm_fn: Optional[Callable[..., None]] = None
                    ) -> torch.Tensor:
    """Block-row distributed C = alpha * A @ B^T + beta * C.

    Shard layout (column-major semantics, tensors in the package's
    (K, cols) convention):
      a_local : (K, M_loc)  rank's block-rows of A       (M split)
      b_local : (K, N_loc)  rank's block-rows of B       (N split)
      c_local : (N, M_loc)  rank's block-rows of C       (M split, full N)

    Every rank needs ALL of B; B is all-gathered K-panel by K-panel and the
    gather of panel p+1 is issued asynchronously before the local GEMM of
    panel p, so RCCL traffic over xGMI overlaps MFMA compute.  `gemm_fn`
    accumulates one panel: gemm_fn(a_panel, b_panel, c_local, alpha, beta).

    batched_gemm_fn (optional): on the gathered path the `world` rank-chunks
    of a panel are a strided batch — a_panel shared, B the stacked
    (world, panel_k, n_loc) gather buffer, C the equally spaced row blocks
    c_local.view(world, n_loc, M_loc) — so when given, one
    batched_gemm_fn(a_panel, buf, c_view, alpha, beta) call per panel
    replaces the loop of `world` gemm_fn calls (ops.ft_sgemm_batched /
    ops.sgemm_batched with a tier bound; torch_batched_gemm_fn on the CPU).
    """
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    k = a_local.shape[0]
    assert b_local.shape[0] == k and k % panel_k == 0
    n_loc = b_local.shape[1]
    npanels = k // panel_k

    # An INITIALIZED world-1 group still takes the collective path below —
    # that is how the RCCL branch (device all_gather_into_tensor consumed by
    # MFMA kernels) is exercised on a single-GPU box (VERDICT r01 next #4a).
    if world == 1 and not dist.is_initialized():
        for p in range(npanels):
            sl = slice(p * panel_k, (p + 1) * panel_k)
            gemm_fn(a_local[sl].contiguous(), b_local[sl].contiguous(),
                    c_local, alpha, beta if p == 0 else 1.0)
        return c_local

    # Two rotating gather buffers so gather(p+1) overlaps compute(p); the
    # stacked (world, panel_k, n_loc) layout is consumed directly — each
    # rank-chunk is a contiguous (panel_k, n_loc) view whose rows are that
    # rank's block of C rows, so no per-panel torch.cat/copy is needed
    # (at N=32768 the concat would move 256 MB per panel inside the timed
    # loop).
    bufs = [torch.empty((world, panel_k, n_loc), dtype=b_local.dtype,
                        device=b_local.device) for _ in range(2)]

    def start_gather(p: int):
        sl = slice(p * panel_k, (p + 1) * panel_k)
        buf = bufs[p & 1]
        work = dist.all_gather_into_tensor(buf.view(world * panel_k, n_loc),
                                           b_local[sl].contiguous(),
                                           group=group, async_op=True)
        return buf, work

    buf, work = start_gather(0)
    for p in range(npanels):
        nxt = start_gather(p + 1) if p + 1 < npanels else None
        work.wait()
        a_panel = a_local[p * panel_k:(p + 1) * panel_k].contiguous()
        b0 = beta if p == 0 else 1.0
        if batched_gemm_fn is not None:
            batched_gemm_fn(a_panel, buf,
                            c_local.view(world, n_loc, c_local.shape[1]),
                            alpha, b0)
        else:
            for rr in range(world):
                # chunk rr covers C rows (= output columns) [rr*n_loc, +n_loc)
                gemm_fn(a_panel, buf[rr],
                        c_local[rr * n_loc:(rr + 1) * n_loc], alpha, b0)
        if nxt is not None:
            buf, work = nxt
    return c_local


def torch_gemm_fn(a_panel, b_panel, c_local, alpha, beta):
    """CPU/GPU plain fp32 panel GEMM for the distributed path (reference
    implementation; the GPU fast path passes ops.ft_sgemm instead).  Like
    the kernels, beta == 0 overwrites C without reading it (0 * NaN would
    keep a NaN of an uninitialised C)."""
    prod = alpha * (b_panel.transpose(0, 1) @ a_panel)
    if beta == 0:
        c_local.copy_(prod)
    else:
        c_local.mul_(beta).add_(prod)


def torch_batched_gemm_fn(a_panel, b_stack, c_stack, alpha, beta):
    """torch.bmm reference of block_row_sgemm's batched_gemm_fn: a_panel
    (panel_k, M_loc) shared, b_stack (world, panel_k, n_loc), c_stack
    (world, n_loc, M_loc) a view of c_local, updated in place.  beta == 0
    overwrites without reading, like torch_gemm_fn."""
    prod = alpha * torch.bmm(
        b_stack.transpose(1, 2),
        a_panel.unsqueeze(0).expand(b_stack.shape[0], -1, -1))
    if beta == 0:
        c_stack.copy_(prod)
    else:
        c_stack.mul_(beta).add_(prod)
