#!/usr/bin/env python3
"""bench.py — flagship benchmark: fused-ABFT SGEMM (abft_kernel_huge) at
N=4096 fp32 on 1..8 MI355X GPUs (weak scaling: one independent GEMM per GPU,
the BASELINE.json headline config).

Driver contract: `python bench.py --gpus N --steps K --warmup W`; for N>1 it
is launched under torch.distributed.run with one rank per GPU (RCCL).  Rank 0
prints ONE JSON line; `value` is the whole-job aggregate GFLOPS over all
ranks, timed as the MAX elapsed over ranks, bracketed by barrier +
torch.cuda.synchronize on both sides.

A "step" is one full fused-ABFT GEMM launch (C = alpha*A*B^T + beta*C at
M=N=K=4096, alpha=1, beta=-1.5, with the always-on 20-fault injector and
in-kernel correction — the reference's headline kernel, BASELINE.md
abft_kernel_huge row).  vs_baseline divides by the reference's published
row for the kernel ACTUALLY selected by --kernel at the size actually run
(abft_kernel_huge 4005 / kernel_sgemm_huge 4792 / cuBLAS 4537 GFLOPS at
N=4096 on T4-class hardware) x n_gpus; the JSON's metric/model/inject
fields likewise reflect the real flags, so a run with --kernel huge or
--kernel rocblas is labeled as the plain kernel it measured.

A plain run does only what the headline figure needs: setup, warmup, the
--steps timed steps, the optional --dump-outputs write, the result line
(`ms_per_step` = milliseconds per timed step).  --dump-outputs DIR saves
the output matrix of the last timed step as float32 .npy for comparing two
builds output for output; --full is where secondary measurements belong
(none exist yet, so it changes nothing).
"""

import argparse
import json
import os
import time

import torch

# Reference published rows (README.md:39-53), per sweep size,
# used so vs_baseline and the JSON labels reflect the kernel ACTUALLY
# benchmarked (--kernel) at the size actually run (--size).
_SWEEP_SIZES = (1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 5120, 5632,
                6144)
_BASELINE_ROWS = {
    "abft_huge": (3811, 4448, 4076, 4024, 3986, 3924, 4005, 3952, 3885, 3955,
                  3945),
    "huge": (4847, 5783, 5020, 4918, 4757, 4742, 4792, 4716, 4730, 4719,
             4721),
    "rocblas": (4695, 5357, 4694, 4647, 4590, 4408, 4537, 4477, 4204, 4453,
                4129),
}
_KERNEL_META = {
    # kernel flag -> (metric name, reference model-row name, inject, faults)
    "abft_huge": ("fused_abft_sgemm_gflops", "abft_kernel_huge", True, 20),
    "huge": ("sgemm_gflops", "kernel_sgemm_huge", False, 0),
    "rocblas": ("sgemm_gflops", "rocblas_sgemm", False, 0),
}


def baseline_gflops_per_gpu(kernel: str, size: int):
    """Reference GFLOPS row entry for this kernel at this sweep size
    (None when the size is not a published sweep point)."""
    if size in _SWEEP_SIZES:
        return float(_BASELINE_ROWS[kernel][_SWEEP_SIZES.index(size)])
    return None


_DUMP_MAX_BYTES = 48 << 20  # per file; keeps a dump well under 64 MB


def dump_output(out_dir: str, name: str, t: torch.Tensor) -> None:
    """Write `t` as out_dir/<name>.npy in float32.  A matrix above the size
    cap is reduced to a fixed sample of whole rows (ascending indices drawn
    by numpy's default_rng(0)), the same rows for every run of that shape."""
    import numpy as np
    arr = t.detach().to("cpu", torch.float32).contiguous().numpy()
    if arr.nbytes > _DUMP_MAX_BYTES:
        arr = arr.reshape(arr.shape[0], -1)
        keep = max(1, _DUMP_MAX_BYTES // (arr.shape[1] * 4))
        rows = np.sort(np.random.default_rng(0).choice(
            arr.shape[0], size=min(keep, arr.shape[0]), replace=False))
        arr = arr[rows]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernel", default="abft_huge",
                    choices=["abft_huge", "huge", "rocblas"])
    ap.add_argument("--mode", default="replicated",
                    choices=["replicated", "blockrow"])
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="cpu: CI smoke of the full multi-rank bench "
                         "contract over gloo (tiny size, torch matmul)")
    ap.add_argument("--graph", action="store_true",
                    help="capture the step in a hipGraph and replay it "
                         "(launch-bound small sizes; replicated mode only "
                         "— the fused path is capture-safe: no syncs, "
                         "stream-ordered workspace, stream-K bypasses "
                         "itself under capture)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the output matrix of "
                         "the LAST timed step to DIR/c.npy (float32; one "
                         "c_rank<r>.npy per rank when multi-rank).  The "
                         "clock is paused before that step to reset C to a "
                         "seeded matrix, so the dump depends only on the "
                         "arguments, not on how many steps ran before")
    ap.add_argument("--full", action="store_true",
                    help="also run the benchmark's secondary measurements; "
                         "there are none yet — a plain run already does "
                         "only setup, warmup, the timed steps and the "
                         "result line — so this is accepted and changes "
                         "nothing")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    cpu_ci = args.device == "cpu"
    if not cpu_ci and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (or --device cpu)")

    from ft_sgemm_amd import ops
    from ft_sgemm_amd.parallel import init_from_env

    rank, world = init_from_env(backend="gloo" if cpu_ci else None)
    import torch.distributed as dist
    dev = (torch.device("cpu") if cpu_ci
           else torch.device("cuda", torch.cuda.current_device()))
    n = args.size
    torch.manual_seed(10 + rank)
    a = (torch.rand((n, n), device=dev) * 1.8 - 0.9).contiguous()
    b = (torch.rand((n, n), device=dev) * 1.8 - 0.9).contiguous()
    c = torch.zeros((n, n), device=dev)

    if args.mode == "blockrow":
        # Block-row distributed SGEMM (BASELINE configs[4b]): A/C sharded by
        # block rows, B K-panels all-gathered over RCCL/xGMI, fused-ABFT
        # MFMA GEMM per local panel, gather(p+1) overlapped with compute(p).
        from ft_sgemm_amd.parallel import block_row_sgemm, local_shard
        mlo, mhi = local_shard(n, rank, world)
        nlo, nhi = local_shard(n, rank, world)
        a_loc = a[:, : mhi - mlo].contiguous()   # synthetic shard (K, M_loc)
        b_loc = b[:, : nhi - nlo].contiguous()   # (K, N_loc)
        c_loc = torch.zeros((n, mhi - mlo), device=dev)
        panel_k = max(1024, n // 16)
        if n % panel_k or panel_k > n:
            panel_k = n  # tiny / odd sizes: single panel

        def gemm_fn(ap, bp, cl, al, be):
            if cpu_ci:
                from ft_sgemm_amd.parallel.distributed import torch_gemm_fn
                torch_gemm_fn(ap, bp, cl, al, be)
            elif args.kernel == "abft_huge":
                ops.ft_sgemm("huge", ap, bp, cl, al, be, inject=True)
            elif args.kernel == "huge":
                ops.sgemm("huge", ap, bp, cl, al, be)
            else:
                ops.rocblas_sgemm(ap, bp, cl, al, be)

        step = lambda: block_row_sgemm(a_loc, b_loc, c_loc, panel_k=panel_k,
                                       gemm_fn=gemm_fn, alpha=1.0, beta=-1.5)
    elif cpu_ci:
        step = lambda: torch.matmul(b.transpose(0, 1), a)
    elif args.kernel == "abft_huge":
        step = lambda: ops.ft_sgemm("huge", a, b, c, 1.0, -1.5, inject=True)
    elif args.kernel == "huge":
        step = lambda: ops.sgemm("huge", a, b, c, 1.0, -1.5)
    else:
        step = lambda: ops.rocblas_sgemm(a, b, c, 1.0, -1.5)

    if args.graph and (cpu_ci or args.mode != "replicated"):
        raise SystemExit("--graph needs --device cuda --mode replicated")

    # the matrix every step updates in place (a caller's result)
    c_out = c_loc if args.mode == "blockrow" else c
    c_seed = None
    if args.dump_outputs:
        # C as the last timed step finds it (drawn after a and b, so the
        # operands are the same with and without the option)
        c_seed = torch.rand_like(c_out) * 1.8 - 0.9

    warm0 = time.perf_counter()
    for _ in range(args.warmup):
        step()
    if not cpu_ci:
        torch.cuda.synchronize()
    # clock-ramp extension: a cold MI355X takes ~1-2 s to reach its steady
    # compute clock; short warmups would time the ramp.  Extra untimed steps
    # (beyond the requested W) are reported in config.warmup_extra.
    warmup_extra = 0
    if not cpu_ci:
        while time.perf_counter() - warm0 < 1.5 and warmup_extra < 2000:
            step()
            warmup_extra += 1
            if warmup_extra % 50 == 0:  # async launches: bound the overshoot
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    if args.graph:
        # capture once on a side stream, then replace step with the replay
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            step()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            step()
        step = g.replay
        g.replay()
        torch.cuda.synchronize()

    if world > 1:
        dist.barrier()
        if not cpu_ci:
            torch.cuda.synchronize()

    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        step()
    paused = 0.0
    if c_seed is not None:
        # stop the clock, give the last step a known C, restart the clock
        if not cpu_ci:
            torch.cuda.synchronize()
        p0 = time.perf_counter()
        c_out.copy_(c_seed)
        if not cpu_ci:
            torch.cuda.synchronize()
        paused = time.perf_counter() - p0
    last = step()
    if not cpu_ci:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0 - paused
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], device="cpu" if cpu_ci else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if not cpu_ci:
            torch.cuda.synchronize()
        elapsed = float(t.item())

    # replicated: every rank computes an independent n^3 GEMM (weak);
    # blockrow: the ranks together compute ONE n^3 GEMM (strong)
    flop_per_step = 2.0 * n * n * n
    mult = 1 if args.mode == "blockrow" else world
    agg_gflops = mult * flop_per_step * args.steps / elapsed / 1e9
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs:
        # the CPU replicated step returns its product instead of updating C
        out = last if cpu_ci and args.mode == "replicated" else c_out
        dump_output(args.dump_outputs,
                    "c" if world == 1 else f"c_rank{rank}", out)

    if rank == 0:
        metric, model, inject, faults = _KERNEL_META[args.kernel]
        base = baseline_gflops_per_gpu(args.kernel, n)
        # replicated weak scaling compares against world x the reference's
        # single-GPU number; blockrow computes ONE GEMM so against 1x.
        vs = (round(agg_gflops / (base * mult), 3) if base is not None
              else None)
        print(json.dumps({
            "metric": metric,
            "value": round(agg_gflops, 1),
            "unit": "GFLOPS",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak" if args.mode == "replicated" else "strong",
            "vs_baseline": vs,
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": model,
                "M": n, "N": n, "K": n,
                "alpha": 1.0, "beta": -1.5,
                "inject": inject, "faults_per_gemm": faults,
                "graph": args.graph,
                "warmup_extra": warmup_extra,
                "parallelism": (f"dp{world}" if args.mode == "replicated"
                                else f"blockrow{world}"),
            },
        }))

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
