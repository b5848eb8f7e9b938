#!/usr/bin/env python3
"""Grouped stream-K against the classic grouped launch, in the style of
tools/bench_grouped.py and tools/bench_ragged_streamk.py: one process, the
arms interleaved within every round, median and spread over the rounds.

Per cell (E experts, tokens split by `counts`, in = out = 1024) one product
of ft_grouped_linear as a GroupedPlan, built once outside the timing (run()
is what a captured launch would replay):
  grad_weight  per expert M = in, N = out, K = counts[e]: few fixed tiles, a
               deep K that differs per expert; the product grouped stream-K
               was built for
  forward      per expert M = out, N = counts[e], K = in, both operands
               transposed: a control, no win is expected
Per path (plain, fused without injection) and stream-K tier:
  classic   the classic grouped launch (streamk=0) on that tier
  classic'  the same plan run again, as an arm of its own: classic / classic'
            is the run-to-run noise of this process (`noise`)
  chosen    the classic launch on ops.choose_tier_grouped's tier
  sk        streamk="auto": the device grid G, plan-owned partials
Times are microseconds per call, median of the rounds, spread =
(max - min) / median.  sk/best = min(classic, chosen) / sk: how many times
faster grouped stream-K is than the better classic arm (below 1.00: it
loses).

  python tools/bench_grouped_streamk.py > profiles/grouped_streamk.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ft_sgemm_amd import ops  # noqa: E402

from bench_grouped import drawn, skewed  # noqa: E402

DIM = 1024  # in = out
# (label, product, counts)
DISTS = [
    ("E=8 T=4096 even", [512] * 8),
    ("E=16 T=4096 halving counts, 4 experts empty", skewed(16, 4096)),
    ("E=64 T=8192 drawn counts", drawn(64, 8192)),
]
CELLS = [(f"grad_weight {lab}", "grad_weight", c) for lab, c in DISTS] + \
    [(f"forward {lab} (control)", "forward", c) for lab, c in DISTS] + \
    [("grad_weight E=8 T=65536 even, deep", "grad_weight", [8192] * 8)]
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


def split(t, counts):
    out, row = [], 0
    for n in counts:
        out.append(t[row:row + n])
        row += n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--cells", default=",".join(map(str, range(len(CELLS)))),
                    help="indices into CELLS")
    args = ap.parse_args()
    print(f"# bench_grouped_streamk: rounds={args.rounds} "
          f"window={args.window}s device={torch.cuda.get_device_name(0)}")
    print("# microseconds per call, median of rounds [spread = "
          "(max-min)/median]; noise = |classic/classic' - 1|; sk/best = "
          "min(classic, chosen) / sk")
    for ci in (int(v) for v in args.cells.split(",")):
        label, product, counts = CELLS[ci]
        experts, tokens = len(counts), sum(counts)
        gen = torch.Generator(device="cpu").manual_seed(10)
        x = (torch.rand((tokens, DIM), generator=gen) * 1.8 - 0.9).cuda()
        gy = (torch.rand((tokens, DIM), generator=gen) * 1.8 - 0.9).cuda()
        w = (torch.rand((experts, DIM, DIM), generator=gen) * 1.8 - 0.9).cuda()
        if product == "grad_weight":
            out = torch.zeros((experts, DIM, DIM), device="cuda")
            lists = (split(x, counts), split(gy, counts), list(out.unbind(0)))
            trans = dict(trans_a=False, trans_b=False)
        else:
            out = torch.zeros((tokens, DIM), device="cuda")
            lists = (list(w.unbind(0)), split(x, counts), split(out, counts))
            trans = dict(trans_a=True, trans_b=True)
        shapes = ops.grouped_layout(*lists, **trans)
        chosen = ops.choose_tier_grouped(shapes)
        flops = 2.0 * DIM * DIM * tokens

        arms, grids, plans = {}, {}, []
        for path, fused in (("plain", False), ("fused", True)):
            def plan(tier, streamk=0):
                p = ops.GroupedPlan(tier, *lists, fused=fused,
                                    streamk=streamk, **trans)
                plans.append(p)
                return p
            arms[(chosen, path, "chosen")] = plan(chosen).run
            for tier in SK_TIERS:
                classic = plan(tier)
                sk = plan(tier, "auto")
                grids[(tier, path)] = sk.streamk_grid
                arms[(tier, path, "classic")] = classic.run
                arms[(tier, path, "classic'")] = classic.run
                arms[(tier, path, "sk")] = sk.run
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

        print(f"\n## {label}: in = out = {DIM}, {flops / 1e9:.1f} GFLOP, "
              f"choose_tier_grouped -> {chosen}\n# counts {counts}")
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
        del x, gy, w, out, lists, arms, plans
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
