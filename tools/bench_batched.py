#!/usr/bin/env python3
"""Strided-batched SGEMM against what it replaces, in the style of
tools/ab_bench.py: one process, variants interleaved within every round,
median and spread over the rounds.

Per shape and per tier that divides it, for the plain and the fused
(no-inject) path:
  loop     a Python loop of `batch` single launches (all one could do before)
  batched  one strided-batched launch
  bmm      torch.bmm on the same operands (printed once per shape)
Every shape is warmed up first; each timing window runs for about --window
seconds.  `spread` is (max - min) / median of a variant's rounds; the last
column says whether batched is slower than loop by more than loop's spread.

  python tools/bench_batched.py > profiles/batched_bmm.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ft_sgemm_amd import ops  # noqa: E402
from ft_sgemm_amd.kernel_table import TIERS, TILING  # noqa: E402

# (label, m, n, k, batch, shared A).  The last is one K panel of
# parallel.block_row_sgemm at world = 8: A shared, B the gathered
# (world, panel_k, n_loc) stack, C equally spaced row blocks.
SHAPES = [
    ("512^3 x64", 512, 512, 512, 64, False),
    ("1024^3 x16", 1024, 1024, 1024, 16, False),
    ("2048^3 x4", 2048, 2048, 2048, 4, False),
    ("block_row panel world=8 (M_loc=1024 n_loc=1024 panel_k=512, shared A)",
     1024, 1024, 512, 8, True),
]


def timed(fn, window):
    """Seconds per call over a window of about `window` seconds."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(window / max(time.perf_counter() - t0, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--tiers", default=",".join(TIERS))
    ap.add_argument("--shapes", default="0,1,2,3",
                    help="indices into SHAPES")
    args = ap.parse_args()
    os.environ.pop("FT_SGEMM_STREAMK", None)  # loop: the shipped auto gate
    tiers = args.tiers.split(",")
    print(f"# bench_batched: rounds={args.rounds} window={args.window}s "
          f"device={torch.cuda.get_device_name(0)}")
    print("# GFLOPS, median of rounds [spread = (max-min)/median]")
    for si in (int(x) for x in args.shapes.split(",")):
        label, m, n, k, batch, shared = SHAPES[si]
        g = torch.Generator(device="cpu").manual_seed(10)
        a = (torch.rand((1 if shared else batch, k, m), generator=g) * 1.8
             - 0.9).cuda()
        b = (torch.rand((batch, k, n), generator=g) * 1.8 - 0.9).cuda()
        c = torch.zeros((batch, n, m), device="cuda")
        a3 = a.expand(batch, k, m)
        flops = 2.0 * m * n * k * batch
        variants = {}
        for tier in tiers:
            t = TILING[tier]
            if m % t["bm"] or n % t["bn"] or k % t["bk"]:
                continue

            def loop_plain(tier=tier):
                for i in range(batch):
                    ops.sgemm(tier, a3[i], b[i], c[i], 1.0, -1.5)

            def loop_fused(tier=tier):
                for i in range(batch):
                    ops.ft_sgemm(tier, a3[i], b[i], c[i], 1.0, -1.5,
                                 inject=False)

            variants[(tier, "plain", "loop")] = loop_plain
            variants[(tier, "plain", "batched")] = (
                lambda tier=tier: ops.sgemm_batched(tier, a3, b, c, 1.0, -1.5))
            variants[(tier, "fused", "loop")] = loop_fused
            variants[(tier, "fused", "batched")] = (
                lambda tier=tier: ops.ft_sgemm_batched(
                    tier, a3, b, c, 1.0, -1.5, inject=False))
        bt = b.transpose(1, 2)
        variants[("-", "-", "bmm")] = lambda: torch.baddbmm(
            c, bt, a3, beta=-1.5, alpha=1.0, out=c)
        for fn in variants.values():  # warm up every variant of the shape
            fn()
            fn()
        torch.cuda.synchronize()
        res = {key: [] for key in variants}
        for _ in range(args.rounds):
            for key, fn in variants.items():
                c.zero_()
                res[key].append(flops / timed(fn, args.window) / 1e9)

        def stat(key):
            v = res[key]
            med = statistics.median(v)
            return med, (max(v) - min(v)) / med

        print(f"\n## {label}")
        med, sp = stat(("-", "-", "bmm"))
        print(f"torch.bmm                       {med:9.0f} [{sp:5.1%}]")
        print(f"{'tier':7s} {'path':6s} {'loop':>9s} {'spread':>8s} "
              f"{'batched':>9s} {'spread':>8s} {'b/loop':>7s}  verdict")
        for tier in tiers:
            for path in ("plain", "fused"):
                if (tier, path, "loop") not in res:
                    continue
                lm, ls = stat((tier, path, "loop"))
                bm_, bs = stat((tier, path, "batched"))
                slower = bm_ < lm * (1.0 - ls)
                print(f"{tier:7s} {path:6s} {lm:9.0f} {ls:8.1%} {bm_:9.0f} "
                      f"{bs:8.1%} {bm_ / lm:7.2f}  "
                      f"{'SLOWER than loop beyond its spread' if slower else 'ok'}",
                      flush=True)


if __name__ == "__main__":
    main()
