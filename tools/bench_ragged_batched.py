#!/usr/bin/env python3
"""Strided-batched ragged SGEMM against what it replaces, in the style of
tools/bench_batched.py: one process, variants interleaved within every round,
median and spread over the rounds.

Per cell, for the tier ops.choose_tier_ragged_batched picks (marked *) and the
alternatives of --alt, for the plain and the fused (no-inject) path:
  loop     a Python loop of `batch` single ragged launches on the same views
           (all one could do before)
  batched  one strided-batched ragged launch
  bmm      torch.baddbmm on the same operands (printed once per cell)
  tiled    ops.sgemm_batched / ops.ft_sgemm_batched, where the tile divides
           the shape (the aligned cell): the launch the ragged batched one is
           expected to be level with
The two attention cells are laid out as ops.ft_bmm lays them out: b is given
transposed, as (N, K) (NT).  Every cell is warmed up first; each timing window
runs for about --window seconds.  `spread` is (max - min) / median of a
variant's rounds; the verdict says whether batched is slower than loop by
more than loop's spread.

  python tools/bench_ragged_batched.py > profiles/ragged_batched.txt
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

# (label, m, n, k, batch, trans_b)
CELLS = [
    ("attention scores x32 (M=N=1000 K=80, NT)", 1000, 1000, 80, 32, True),
    ("attention context x32 (M=80 N=1000 K=1000, NT)", 80, 1000, 1000, 32,
     True),
    ("1025^3 x16", 1025, 1025, 1025, 16, False),
    ("1024^3 x16 (aligned)", 1024, 1024, 1024, 16, False),
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
    ap.add_argument("--alt", default="huge,large,medium",
                    help="tiers run next to the chosen one")
    ap.add_argument("--cells", default="0,1,2,3", help="indices into CELLS")
    args = ap.parse_args()
    print(f"# bench_ragged_batched: rounds={args.rounds} "
          f"window={args.window}s device={torch.cuda.get_device_name(0)}")
    print("# GFLOPS, median of rounds [spread = (max-min)/median]; "
          "* = choose_tier_ragged_batched")
    for ci in (int(x) for x in args.cells.split(",")):
        label, m, n, k, batch, tb = CELLS[ci]
        chosen = ops.choose_tier_ragged_batched(m, n, k, batch)
        tiers = [t for t in TIERS if t == chosen or t in args.alt.split(",")]
        g = torch.Generator(device="cpu").manual_seed(10)
        a = (torch.rand((batch, k, m), generator=g) * 1.8 - 0.9).cuda()
        b = (torch.rand((batch, k, n), generator=g) * 1.8 - 0.9).cuda()
        bt = b.transpose(1, 2)  # (B, N, K) view: torch.bmm's left operand
        bk = bt.contiguous() if tb else b  # what the kernels are handed
        c = torch.zeros((batch, n, m), device="cuda")
        flops = 2.0 * m * n * k * batch
        kw = dict(trans_b=tb)
        variants = {}
        for tier in tiers:
            def loop_plain(tier=tier):
                for i in range(batch):
                    ops.sgemm_ragged(tier, a[i], bk[i], c[i], 1.0, -1.5, **kw)

            def loop_fused(tier=tier):
                for i in range(batch):
                    ops.ft_sgemm_ragged(tier, a[i], bk[i], c[i], 1.0, -1.5,
                                        inject=False, **kw)

            variants[(tier, "plain", "loop")] = loop_plain
            variants[(tier, "plain", "batched")] = (
                lambda tier=tier: ops.sgemm_ragged_batched(
                    tier, a, bk, c, 1.0, -1.5, **kw))
            variants[(tier, "fused", "loop")] = loop_fused
            variants[(tier, "fused", "batched")] = (
                lambda tier=tier: ops.ft_sgemm_ragged_batched(
                    tier, a, bk, c, 1.0, -1.5, inject=False, **kw))
            t = TILING[tier]
            if not (tb or m % t["bm"] or n % t["bn"] or k % t["bk"]):
                variants[(tier, "plain", "tiled")] = (
                    lambda tier=tier: ops.sgemm_batched(tier, a, b, c, 1.0,
                                                        -1.5))
                variants[(tier, "fused", "tiled")] = (
                    lambda tier=tier: ops.ft_sgemm_batched(
                        tier, a, b, c, 1.0, -1.5, inject=False))
        variants[("-", "-", "bmm")] = lambda: torch.baddbmm(
            c, bt, a, beta=-1.5, alpha=1.0, out=c)
        for fn in variants.values():  # warm up every variant of the cell
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
        print(f"torch.bmm                        {med:9.0f} [{sp:5.1%}]")
        print(f"{'tier':8s} {'path':6s} {'loop':>9s} {'spread':>8s} "
              f"{'batched':>9s} {'spread':>8s} {'b/loop':>7s} "
              f"{'tiled':>9s} {'spread':>8s} {'b/tiled':>7s}  verdict")
        for tier in tiers:
            for path in ("plain", "fused"):
                lm, ls = stat((tier, path, "loop"))
                bm_, bs = stat((tier, path, "batched"))
                if (tier, path, "tiled") in res:
                    tm, ts = stat((tier, path, "tiled"))
                    tiled = f"{tm:9.0f} {ts:8.1%} {bm_ / tm:7.2f}"
                else:
                    tiled = f"{'-':>9s} {'-':>8s} {'-':>7s}"
                slower = bm_ < lm * (1.0 - ls)
                name = tier + ("*" if tier == chosen else "")
                print(f"{name:8s} {path:6s} {lm:9.0f} {ls:8.1%} {bm_:9.0f} "
                      f"{bs:8.1%} {bm_ / lm:7.2f} {tiled}  "
                      f"{'SLOWER than loop beyond its spread' if slower else 'ok'}",
                      flush=True)


if __name__ == "__main__":
    main()
