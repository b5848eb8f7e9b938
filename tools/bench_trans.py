#!/usr/bin/env python3
"""Transposed-operand ragged SGEMM against what it replaces.

For y (N, M) = b (N, K) @ a (M, K)^T — a linear layer's forward product, both
operands row-major with K inner — on the huge tier, plain and fused
(no-inject), four routes:
  tt       the TT call on the operands as they lie
  copies   two .t().contiguous() copies plus the untransposed ragged call,
           the copies inside the timed region (all one could do before)
  pre      the untransposed ragged call on operands transposed beforehand
           (the ceiling)
  linear   torch.nn.functional.linear (context, printed with plain only)
and, for the fast register path alone:
  tt_guarded  the TT call on 4-byte-offset, odd-row-stride views, which
              takes the guarded staging path everywhere
Device-event timings, every shape warmed up, variants interleaved within
every round, median and spread = (max - min) / median over the rounds.
Run under a time limit:

  timeout 600 python tools/bench_trans.py > profiles/trans.txt

The lane map of the fast path is a compile-time choice
(FT_TRANS_ROW_FASTEST, csrc/ft_ragged.hpp): build once with and once
without and run this tool on each.  Segment-sum kernel times come from a
kernel trace of --trace-run, not from this tool's timings.
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ft_sgemm_amd import ops  # noqa: E402

# (label, tokens = N, out = M, in = K)
SHAPES = [("4096^3", 4096, 4096, 4096),
          ("layer tokens=8192 in=out=4096", 8192, 4096, 4096)]
TIER = "huge"


def timed(fn, reps):
    """Milliseconds per call by device events around `reps` calls."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def offset_strided(x):
    r, c = x.shape
    ld = c + 1 + c % 2
    flat = torch.zeros(r * ld + 1, device=x.device)
    view = flat.as_strided((r, c), (ld, 1), 1)
    view.copy_(x)
    return view


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--trace-run", action="store_true",
                    help="a few fused TN and untransposed calls at 4096^3 "
                         "and nothing else, for a kernel trace")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.have_extension()
    if args.trace_run:
        g = torch.Generator(device="cpu").manual_seed(10)
        a = (torch.rand((4096, 4096), generator=g) * 1.8 - 0.9).cuda()
        c = torch.zeros((4096, 4096), device="cuda")
        for _ in range(5):
            ops.ft_sgemm_ragged(TIER, a, a, c, inject=False)
            ops.ft_sgemm_ragged(TIER, a, a, c, inject=False, trans_a=True)
        torch.cuda.synchronize()
        return
    print(f"# bench_trans: tier={TIER} rounds={args.rounds} reps={args.reps} "
          f"device={torch.cuda.get_device_name(0)}")
    print("# ms per call, median of rounds [spread]; GFLOPS of the median")
    for si in (int(s) for s in args.shapes.split(",")):
        label, n, m, k = SHAPES[si]
        g = torch.Generator(device="cpu").manual_seed(10)
        w = (torch.rand((m, k), generator=g) * 1.8 - 0.9).cuda()  # a, (M, K)
        x = (torch.rand((n, k), generator=g) * 1.8 - 0.9).cuda()  # b, (N, K)
        c = torch.zeros((n, m), device="cuda")
        wt, xt = w.t().contiguous(), x.t().contiguous()
        wo, xo, co = offset_strided(w), offset_strided(x), offset_strided(c)
        flops = 2.0 * m * n * k
        for mode in ("plain", "fused"):
            def call(a, b, out, ta, tb):
                if mode == "plain":
                    ops.sgemm_ragged(TIER, a, b, out, trans_a=ta, trans_b=tb)
                else:
                    ops.ft_sgemm_ragged(TIER, a, b, out, inject=False,
                                        trans_a=ta, trans_b=tb)
            routes = {
                "tt": lambda: call(w, x, c, True, True),
                "copies": lambda: call(w.t().contiguous(),
                                       x.t().contiguous(), c, False, False),
                "pre": lambda: call(wt, xt, c, False, False),
                "tt_guarded": lambda: call(wo, xo, co, True, True),
            }
            if mode == "plain":
                routes["linear"] = lambda: F.linear(x, w)
            # results must agree before speeds are compared
            call(w, x, c, True, True)
            want = c.clone()
            call(wt, xt, c, False, False)
            assert torch.equal(c, want), "tt differs from pre"
            for fn in routes.values():  # warm-up
                timed(fn, 2)
            ms = {name: [] for name in routes}
            for _ in range(args.rounds):
                for name, fn in routes.items():
                    ms[name].append(timed(fn, args.reps))
            print(f"{label}  {mode}")
            for name, v in ms.items():
                med = statistics.median(v)
                print(f"  {name:11s} {med:8.3f} ms  [{(max(v) - min(v)) / med:5.1%}]"
                      f"  {flops / med / 1e6:9.0f} GFLOPS")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
