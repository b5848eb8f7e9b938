#!/usr/bin/env python3
"""Library usage examples (run on a ROCm GPU box).

Tensor convention: a column-major MxK fp32 matrix is a contiguous (K, M)
CUDA tensor (same bytes, zero copies) — see ft_sgemm_amd/__init__.py.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ft_sgemm_amd import ops

# --- operands: C = alpha * A @ B^T + beta * C, A (MxK), B (NxK), C (MxN)
m = n = k = 4096
a, b, c = ops.make_operands(m, n, k)          # uniform (-0.9, 0.9), seed 10

# 1. plain hand-tiled MFMA SGEMM, explicit tier
ops.sgemm("huge", a, b, c, alpha=1.0, beta=0.0)

# 2. fused-ABFT SGEMM with the always-on 20-fault self-test: every fault is
#    detected, located (ratio locate) and corrected in-kernel; the result
#    still matches the clean product
ops.ft_sgemm("huge", a, b, c, alpha=1.0, beta=0.0, inject=True)

# 2b. the same, with a fault report: which element, which k window, was it
#     corrected.  A report accumulates across launches until reset();
#     read() is the only call that synchronises.
report = ops.FaultReport(capacity=1024)
ops.ft_sgemm("huge", a, b, c, alpha=1.0, beta=0.0, inject=True, report=report)
r = report.read()
print(f"faults: tripped {r.tripped} corrected {r.corrected} uncorrected "
      f"{r.uncorrected} unlocated {r.unlocated} (dropped {r.dropped})")
print("first event:", r.events[0])
report.raise_if_uncorrected()   # refuse a result that could not be repaired
report.reset()

# 3. automatic tier selection (grid-fill aware)
ops.ft_sgemm_auto(a, b, c)

# 4. vendor-BLAS oracle and the non-fused rocBLAS ABFT baseline
ops.rocblas_sgemm(a, b, c)
c2, (res_row, res_col) = ops.baseline_ft(a, b, c, panel_k=1024)
print("baseline verdicts (squared residual norms):", res_row, res_col)

# 5. reference-id dispatch (0=rocBLAS, 1-6 plain, 10 baseline, 11-16 fused)
ops.run_kernel_id(16, a, b, c)

# 5b. stream-K control: the launcher auto-selects the stream-K twin at
#     grid-straggler sizes (measured gates); force / disable explicitly:
os.environ["FT_SGEMM_STREAMK"] = "1"   # force (pipelined callers win from
ops.sgemm("huge", a, b, c)             # N>=1024 up); "0" disables; unset
os.environ.pop("FT_SGEMM_STREAMK")     # = auto

# 5c. odd shapes fall back to rocBLAS (FT entry adds the offline ABFT
#     verdict chain) instead of raising
ao, bo, co = ops.make_operands(100, 257, 65)
ops.ft_sgemm_auto(ao, bo, co)

# 6. distributed block-row SGEMM (one process per GPU over RCCL; see
#    bench.py --mode blockrow for the full multi-rank setup)
from ft_sgemm_amd.parallel import block_row_sgemm

block_row_sgemm(a, b, c, panel_k=1024,
                gemm_fn=lambda ap, bp, cl, al, be:
                    ops.ft_sgemm("huge", ap, bp, cl, al, be, inject=True))

# 7. strided batch: 16 independent 1024^3 products in ONE launch (plus one
#    checksum-encode launch).  a:(B,K,M) b:(B,K,N) c:(B,N,M); a 2-D or
#    expand()ed operand is shared by all entries, padded batch strides are
#    fine (multiples of 4 floats).  One fault log per entry.
ab = torch.rand((16, 1024, 1024), device="cuda")
bb = torch.rand((16, 1024, 1024), device="cuda")
cb = torch.zeros((16, 1024, 1024), device="cuda")
ops.sgemm_batched("large", ab, bb, cb)
breport = ops.BatchedFaultReport(batch=16)
ops.ft_sgemm_batched("large", ab[0], bb, cb, inject=True, report=breport)
print("per-entry corrected faults:", [r.corrected for r in breport.read()])
breport.raise_if_uncorrected()  # names the entries it could not repair

#    the distributed path's per-rank-chunk loop is such a batch:
block_row_sgemm(a, b, c, panel_k=1024,
                gemm_fn=lambda ap, bp, cl, al, be:
                    ops.ft_sgemm("huge", ap, bp, cl, al, be, inject=True),
                batched_gemm_fn=lambda ap, bs, cs, al, be:
                    ops.ft_sgemm_batched("huge", ap, bs, cs, al, be))

# 8. transposed operands: a linear layer's y = x @ W^T has both operands
#    row-major with K inner — trans_a / trans_b read them in place (ragged
#    entries only), with the bits of the call on .t().contiguous() copies.
x = torch.rand((1000, 515), device="cuda")        # (tokens, in)  = b as (N, K)
w = torch.rand((777, 515), device="cuda")         # (out, in)     = a as (M, K)
y = torch.empty((1000, 777), device="cuda")       # (tokens, out) = c   (N, M)
ops.ft_sgemm_ragged("large", w, x, y, inject=True, trans_a=True, trans_b=True)

#    the same as a differentiable layer: forward, grad_x and grad_weight all
#    run the fused-ABFT kernel with no operand copy; one report for all three
lin = ops.FTLinear(515, 777, device="cuda", inject=True, report=report)
lin(x.requires_grad_()).sum().backward()
print("linear layer corrected faults:", report.read().corrected)

# 9. batched matrix product: attention scores for 12 heads of dimension 80 on
#    head views of one (T, heads, 80) projection output.  ft_bmm reads the
#    (heads, T, 80) views and the transposed keys in place (no copy) and runs
#    forward and both backward products as one fused-ABFT ragged batched
#    launch each; one BatchedFaultReport, a slot per head, for all three.
q = torch.rand((1000, 12, 80), device="cuda", requires_grad=True)
k = torch.rand((1000, 12, 80), device="cuda", requires_grad=True)
hreport = ops.BatchedFaultReport(batch=12)
scores = ops.ft_bmm(q.permute(1, 0, 2), k.permute(1, 0, 2).transpose(1, 2),
                    inject=True, report=hreport)   # (12, 1000, 1000)
scores.sum().backward()
print("per-head corrected faults:", [r.corrected for r in hreport.read()])
hreport.raise_if_uncorrected()

# 10. grouped launch: products with their own shapes in ONE launch.  The
#     expert layer of a mixture-of-experts block is such a group: the rows of
#     x are sorted by expert, counts (on the host) says how many each expert
#     owns, one of them none.  Forward, grad_x and grad_weight are one
#     fused-ABFT grouped launch each; the empty expert gets a zero grad_weight.
counts = [700, 0, 37, 263]
xe = torch.rand((sum(counts), 515), device="cuda", requires_grad=True)
we = torch.rand((4, 777, 515), device="cuda", requires_grad=True)
ereport = ops.BatchedFaultReport(batch=4)
ye = ops.ft_grouped_linear(xe, we, counts, inject=True, report=ereport)
ye.sum().backward()
print("per-expert corrected faults:", [r.corrected for r in ereport.read()])
assert not we.grad[1].any()
#     the launch itself, on any list of (a, b, c): a plan uploads the
#     descriptor table once, run() launches with no allocation or sync
ws_, xs_ = list(we.detach().unbind(0)), list(xe.detach().split(counts))
ys_ = [torch.empty((n, 777), device="cuda") for n in counts]
plan = ops.GroupedPlan("large", ws_, xs_, ys_, fused=True, trans_a=True,
                       trans_b=True)
plan.run(1.0, 0.0)

torch.cuda.synchronize()
print("examples OK")
