#!/usr/bin/env python3
"""Grouped ragged SGEMM against what it replaces, on the three products of a
mixture-of-experts layer (ops.ft_grouped_linear's mapping), in the style of
tools/bench_ragged_batched.py: one process, variants interleaved within every
round, median and spread over the rounds.

Per cell (E experts, T tokens split by `counts`, in, out) and per product
(forward TT, grad_x NT, grad_weight NN), on the tier ops.choose_tier_grouped
picks and on --alt, for the plain and the fused (no-inject) path:
  grouped  GroupedPlan.run: one launch (fused: plus one encode launch)
  loop     a Python loop of single ragged launches over the experts that have
           tokens (all one could do before without padding)
  padded   one strided-batched ragged launch on operands padded with zeros to
           the largest expert (the copies into the padded buffers are made
           once, outside the timing)
  torch    a loop of torch.nn.functional.linear / matmul (once per product)
`build` is the time to make a GroupedPlan (layout check, table build, upload,
workspace allocation), which one-shot calls pay every time and run() never.
Times are microseconds per call, median of the rounds, spread =
(max - min) / median.  Useful GFLOPS count the real tokens only.

  python tools/bench_grouped.py > profiles/grouped.txt
"""

import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ft_sgemm_amd import ops  # noqa: E402
from ft_sgemm_amd.kernel_table import TIERS  # noqa: E402


def skewed(experts, tokens):
    """Halving counts, the last quarter of the experts empty."""
    live = experts - experts // 4
    counts = [tokens >> (e + 1) for e in range(live)]
    counts[live - 1] += tokens - sum(counts)
    return counts + [0] * (experts - live)


def drawn(experts, tokens, seed=3):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.multinomial(torch.rand(experts, generator=g) ** 2, tokens,
                            replacement=True, generator=g)
    return torch.bincount(ids, minlength=experts).tolist()


# (label, experts, tokens, in, out, counts)
CELLS = [
    ("E=8 T=4096 in=1024 out=1024, even", 8, 4096, 1024, 1024, [512] * 8),
    ("E=16 T=4096 in=512 out=1024, halving counts, 4 experts empty", 16, 4096,
     512, 1024, skewed(16, 4096)),
    ("E=64 T=8192 in=256 out=512, drawn counts", 64, 8192, 256, 512,
     drawn(64, 8192)),
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


def split(t, counts):
    out, row = [], 0
    for n in counts:
        out.append(t[row:row + n])
        row += n
    return out


def padded(t, counts):
    """(E, max count, width) zero-padded copy of the experts' rows of t."""
    out = torch.zeros((len(counts), max(counts), t.shape[1]), device=t.device)
    for e, part in enumerate(split(t, counts)):
        out[e, :part.shape[0]] = part
    return out


def products(x, w, g, counts):
    """Per product: (name, trans_a, trans_b, a_list, b_list, c_list, batched
    (a, b, c) on padded operands, torch loop, useful flops)."""
    experts, out, inner = w.shape
    tokens = x.shape[0]
    y = torch.zeros((tokens, out), device="cuda")
    gx = torch.zeros_like(x)
    gw = torch.zeros_like(w)
    xs, gs, ys, gxs = (split(t, counts) for t in (x, g, y, gx))
    ws, gws = list(w.unbind(0)), list(gw.unbind(0))
    xp, gp = padded(x, counts), padded(g, counts)
    yp = torch.zeros((experts, max(counts), out), device="cuda")
    gxp = torch.zeros((experts, max(counts), inner), device="cuda")
    live = [e for e in range(experts) if counts[e]]
    flops = 2.0 * tokens * inner * out

    def t_fwd():
        for e in live:
            F.linear(xs[e], ws[e])

    def t_gx():
        for e in live:
            torch.matmul(gs[e], ws[e])

    def t_gw():
        for e in live:
            torch.matmul(gs[e].t(), xs[e])

    return [
        ("forward (TT, N varies)", True, True, ws, xs, ys, (w, xp, yp), t_fwd,
         flops),
        ("grad_x (NT, N varies)", False, True, ws, gs, gxs, (w, gp, gxp),
         t_gx, flops),
        ("grad_weight (NN, K varies)", False, False, xs, gs, gws,
         (xp, gp, gw), t_gw, flops),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--alt", default="", help="tiers run next to the chosen "
                    "one, comma separated")
    ap.add_argument("--cells", default="0,1,2", help="indices into CELLS")
    args = ap.parse_args()
    print(f"# bench_grouped: rounds={args.rounds} window={args.window}s "
          f"device={torch.cuda.get_device_name(0)}")
    print("# microseconds per call, median of rounds [spread = "
          "(max-min)/median]; * = choose_tier_grouped; encode grid: "
          "(largest entry, entries) with early exit")
    for ci in (int(v) for v in args.cells.split(",")):
        label, experts, tokens, inner, out, counts = CELLS[ci]
        assert sum(counts) == tokens and len(counts) == experts
        gen = torch.Generator(device="cpu").manual_seed(10)
        r = lambda *s: (torch.rand(s, generator=gen) * 1.8 - 0.9).cuda()  # noqa
        x, w, g = r(tokens, inner), r(experts, out, inner), r(tokens, out)
        print(f"\n## {label}\n# counts {counts}")
        for (name, ta, tb, al, bl, cl, (pa, pb, pc), torch_loop,
             flops) in products(x, w, g, counts):
            kw = dict(trans_a=ta, trans_b=tb)
            shapes = ops.grouped_layout(al, bl, cl, ta, tb)
            chosen = ops.choose_tier_grouped(shapes)
            tiers = [t for t in TIERS
                     if t == chosen or t in args.alt.split(",")]
            live = [e for e, s in enumerate(shapes) if min(s[:3]) > 0]
            variants, builds = {("-", "-", "torch"): torch_loop}, {}
            for tier in tiers:
                for path, fused in (("plain", False), ("fused", True)):
                    plan = ops.GroupedPlan(tier, al, bl, cl, fused=fused, **kw)
                    variants[(tier, path, "grouped")] = (
                        lambda plan=plan: plan.run(1.0, 0.0))
                    builds[(tier, path)] = (
                        lambda tier=tier, fused=fused: ops.GroupedPlan(
                            tier, al, bl, cl, fused=fused, **kw))

                    def loop(tier=tier, fused=fused):
                        for e in live:
                            if fused:
                                ops.ft_sgemm_ragged(tier, al[e], bl[e], cl[e],
                                                    1.0, 0.0, inject=False,
                                                    **kw)
                            else:
                                ops.sgemm_ragged(tier, al[e], bl[e], cl[e],
                                                 1.0, 0.0, **kw)

                    variants[(tier, path, "loop")] = loop
                    call = (ops.ft_sgemm_ragged_batched if fused
                            else ops.sgemm_ragged_batched)
                    pkw = dict(kw, inject=False) if fused else kw
                    variants[(tier, path, "padded")] = (
                        lambda call=call, tier=tier, pkw=pkw: call(
                            tier, pa, pb, pc, 1.0, 0.0, **pkw))
            for fn in variants.values():  # warm up every variant
                fn()
                fn()
            torch.cuda.synchronize()
            res = {key: [] for key in list(variants) + [
                (t, p, "build") for t, p in builds]}
            for _ in range(args.rounds):
                for key, fn in variants.items():
                    res[key].append(timed(fn, args.window) * 1e6)
                for (t, p), fn in builds.items():
                    res[(t, p, "build")].append(timed(fn, args.window) * 1e6)

            def stat(key):
                v = res[key]
                med = statistics.median(v)
                return med, (max(v) - min(v)) / med

            tm, ts = stat(("-", "-", "torch"))
            print(f"\n### {name}: {flops / 1e9:.2f} useful GFLOP")
            print(f"torch loop {tm:9.1f} us [{ts:5.1%}] "
                  f"{flops / tm / 1e3:8.0f} GFLOPS")
            print(f"{'tier':8s} {'path':6s} {'grouped':>9s} {'spread':>7s} "
                  f"{'GFLOPS':>8s} {'loop':>9s} {'spread':>7s} {'padded':>9s} "
                  f"{'spread':>7s} {'build':>9s} {'g/loop':>7s} "
                  f"{'g/padded':>8s} {'g/torch':>8s}")
            for tier in tiers:
                for path in ("plain", "fused"):
                    gm, gs_ = stat((tier, path, "grouped"))
                    lm, ls = stat((tier, path, "loop"))
                    pm, ps = stat((tier, path, "padded"))
                    bm, _ = stat((tier, path, "build"))
                    nm = tier + ("*" if tier == chosen else "")
                    print(f"{nm:8s} {path:6s} {gm:9.1f} {gs_:7.1%} "
                          f"{flops / gm / 1e3:8.0f} {lm:9.1f} {ls:7.1%} "
                          f"{pm:9.1f} {ps:7.1%} {bm:9.1f} {lm / gm:7.2f} "
                          f"{pm / gm:8.2f} {tm / gm:8.2f}", flush=True)
    print("\n# g/loop, g/padded, g/torch: how many times faster the grouped "
          "launch is (below 1.00: it loses)")


if __name__ == "__main__":
    main()
