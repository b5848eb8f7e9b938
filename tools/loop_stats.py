#!/usr/bin/env python3
"""Wait structure of the K-panel loop, read from gfx950 assembly.

Usage:
    hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -Icsrc \
        --cuda-device-only -S csrc/generated/kernel_huge.hip -o huge.s
    python3 tools/loop_stats.py huge.s [more.s ...]

Per GEMM kernel in the file, the basic block holding the most MFMAs is
taken as the panel loop body and one table row is printed: VGPRs, scratch
bytes, full LGKM drains (`s_waitcnt ... lgkmcnt(0)`), counted LGKM waits,
MFMAs before / after `s_barrier`, `v_mov_b32` and LDS reads in that block.
This is the table of docs/ABLATION.md §5b.
"""
import re
import sys


def kernels(text):
    """Yield (name, body lines) per .type @function symbol."""
    cur, body = None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            if cur:
                yield cur, body
            cur, body = m.group(1), []
        elif cur:
            if line.startswith("\t.section") or ".end_amdhsa_kernel" in line:
                yield cur, body
                cur, body = None, []
            else:
                body.append(line)
    if cur:
        yield cur, body


def blocks(body):
    blk = []
    for line in body:
        if re.match(r"^\.LBB\d+_\d+:", line):
            yield blk
            blk = []
        blk.append(line)
    yield blk


def short(name):
    m = re.search(r"(sgemm_mfma\w*?)ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)"
                  r"ELi(\d+)ELb(\d)ELb(\d)", name)
    if not m:
        return None
    k = "sk" if "streamk" in m.group(1) else "classic"
    bm, bn, bk, wm, wn, mm, abft, inj = m.groups()[1:]
    v = "plain" if abft == "0" else ("fused+inj" if inj == "1" else "fused")
    return f"{k} {bm}x{bn}x{bk} w{wm}x{wn} {v}"


def main():
    print("| kernel | VGPR | scratch B | lgkmcnt(0) | counted lgkm | "
          "MFMA before/after barrier | v_mov_b32 | ds_read |")
    print("|---|---|---|---|---|---|---|---|")
    for path in sys.argv[1:]:
        text = open(path).read()
        meta = {}
        for m in re.finditer(
                r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:"
                r"\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
            meta[m.group(1)] = (int(m.group(3)), int(m.group(2)))
        for name, body in kernels(text):
            label = short(name)
            if label is None:
                continue
            best = max(blocks(body),
                       key=lambda b: sum("v_mfma" in x for x in b))
            bar = next((i for i, x in enumerate(best) if "s_barrier" in x),
                       len(best))
            mf = [i for i, x in enumerate(best) if "v_mfma" in x]
            waits = [x for x in best if "s_waitcnt" in x and "lgkmcnt" in x]
            full = sum("lgkmcnt(0)" in x for x in waits)
            vg, sc = meta.get(name, (-1, -1))
            print(f"| {label} | {vg} | {sc} | {full} | {len(waits) - full} | "
                  f"{sum(i < bar for i in mf)}/{sum(i > bar for i in mf)} | "
                  f"{sum('v_mov_b32' in x for x in best)} | "
                  f"{sum('ds_read' in x for x in best)} |")


if __name__ == "__main__":
    main()
