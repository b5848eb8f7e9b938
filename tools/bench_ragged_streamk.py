#!/usr/bin/env python3
"""Ragged stream-K against the classic ragged launch, in the style of
tools/bench_grouped.py: one process, the arms interleaved within every round,
median and spread over the rounds.

Per cell (M, N, K; operands as ops.sgemm_ragged takes them, untransposed) and
per path (plain, fused without injection), for each stream-K tier:
  classic   ops.sgemm_ragged / ft_sgemm_ragged with streamk=0 on that tier
  classic'  the same call again, as an arm of its own: classic / classic' is
            the run-to-run noise of this process (`noise`)
  chosen    the classic launch on ops.choose_tier(m, n, k, ragged=True)'s tier
  sk        streamk at the device grid G, partials allocated once outside the
            timing (the call is what a captured launch would replay)
  torch     torch.matmul, once per cell, for context
Times are microseconds per call, median of the rounds, spread =
(max - min) / median.  sk/best = min(classic, chosen) / sk: how many times
faster stream-K is than the better classic arm (below 1.00: it loses).

  python tools/bench_ragged_streamk.py > profiles/ragged_streamk.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ft_sgemm_amd import ops  # noqa: E402

# (label, M, N, K)
CELLS = [
    ("grad_weight 1024x1024, K = 16384 tokens", 1024, 1024, 16384),
    ("grad_weight 1024x1024, K = 65536 tokens", 1024, 1024, 65536),
    ("grad_weight 1000x1000, K = 16385 tokens", 1000, 1000, 16385),
    ("straggler 4097x4097x4096 (huge: 561 tiles, 512 slots)", 4097, 4097,
     4096),
    ("3073^3", 3073, 3073, 3073),
    ("control 4096x4096x8192 (fills the chip)", 4096, 4096, 8192),
]
SK_TIERS = ("huge", "large")


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--cells", default=",".join(map(str, range(len(CELLS)))),
                    help="indices into CELLS")
    args = ap.parse_args()
    print(f"# bench_ragged_streamk: rounds={args.rounds} "
          f"window={args.window}s device={torch.cuda.get_device_name(0)}")
    print("# microseconds per call, median of rounds [spread = "
          "(max-min)/median]; noise = |classic/classic' - 1|; sk/best = "
          "min(classic, chosen) / sk")
    for ci in (int(v) for v in args.cells.split(",")):
        label, m, n, k = CELLS[ci]
        gen = torch.Generator(device="cpu").manual_seed(10)
        a = (torch.rand((k, m), generator=gen) * 1.8 - 0.9).cuda()
        b = (torch.rand((k, n), generator=gen) * 1.8 - 0.9).cuda()
        c = torch.zeros((n, m), device="cuda")
        chosen = ops.choose_tier(m, n, k, ragged=True)
        flops = 2.0 * m * n * k
        bt = b.t().contiguous()

        def call(tier, fused, **kw):
            if fused:
                return lambda: ops.ft_sgemm_ragged(tier, a, b, c, 1.0, 0.0,
                                                   inject=False, **kw)
            return lambda: ops.sgemm_ragged(tier, a, b, c, 1.0, 0.0, **kw)

        arms = {("-", "-", "torch"): lambda: torch.matmul(bt, a)}
        grids = {}
        for path, fused in (("plain", False), ("fused", True)):
            arms[(chosen, path, "chosen")] = call(chosen, fused)
            for tier in SK_TIERS:
                g = ops._C.ragged_streamk_grid(ops.tier_index(tier), fused,
                                               False, m, n, k)
                grids[(tier, path)] = g
                partials = torch.empty(ops.streamk_partials_floats(tier, g),
                                       device="cuda")
                arms[(tier, path, "classic")] = call(tier, fused)
                arms[(tier, path, "classic'")] = call(tier, fused)
                arms[(tier, path, "sk")] = call(tier, fused, streamk=g,
                                                partials=partials)
        for fn in arms.values():  # warm up every arm
            fn()
            fn()
        torch.cuda.synchronize()
        res = {key: [] for key in arms}
        for _ in range(args.rounds):
            for key, fn in arms.items():
                res[key].append(timed(fn, args.window) * 1e6)

        def stat(key):
            v = res[key]
            med = statistics.median(v)
            return med, (max(v) - min(v)) / med

        tm, ts = stat(("-", "-", "torch"))
        print(f"\n## {label}: {flops / 1e9:.1f} GFLOP, choose_tier -> "
              f"{chosen}")
        print(f"torch.matmul {tm:9.1f} us [{ts:5.1%}] "
              f"{flops / tm / 1e6:7.1f} TF")
        print(f"{'tier':6s} {'path':6s} {'G':>5s} {'classic':>9s} "
              f"{'spread':>7s} {'noise':>6s} {'chosen':>9s} {'spread':>7s} "
              f"{'sk':>9s} {'spread':>7s} {'sk TF':>7s} {'sk/classic':>10s} "
              f"{'sk/best':>8s}")
        for tier in SK_TIERS:
            for path in ("plain", "fused"):
                cm, cs = stat((tier, path, "classic"))
                c2, _ = stat((tier, path, "classic'"))
                hm, hs = stat((chosen, path, "chosen"))
                sm, ss = stat((tier, path, "sk"))
                print(f"{tier:6s} {path:6s} {grids[(tier, path)]:5d} "
                      f"{cm:9.1f} {cs:7.1%} {abs(cm / c2 - 1):6.1%} "
                      f"{hm:9.1f} {hs:7.1%} {sm:9.1f} {ss:7.1%} "
                      f"{flops / sm / 1e6:7.1f} {cm / sm:10.2f} "
                      f"{min(cm, hm) / sm:8.2f}", flush=True)
        del a, b, c, bt, arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
