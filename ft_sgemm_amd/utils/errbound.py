"""fp64 reference and derived elementwise error bound of the SGEMM
C = alpha * A B^T + beta * C0, in the package's storage convention
(a: (K, M), b: (K, N), c: (N, M) tensors).

The bound is the standard componentwise one for K fp32 fused multiply-adds
summed in ANY order,

    E = (K + 8) * 2**-23 * (|alpha| * (P + extra) + |beta| * |C0|),
    P = |B| |A|^T,

with 2**-23 per operation (covers truncating as well as round-to-nearest
accumulation; the MFMA's internal rounding is not assumed), and +8 for the
alpha/beta epilogue and the few extra adds of a stream-K slot sum.  Nothing
in it is tuned: any correct fp32 kernel satisfies it.  `extra` is an
additional magnitude carried through the accumulation (e.g. an injected
fault that is meant to stay in the result).
"""

from __future__ import annotations

import torch

EPS = 2.0 ** -23


def ref64(a: torch.Tensor, b: torch.Tensor, c0, alpha: float,
          beta: float) -> torch.Tensor:
    """alpha * (b^T a) + beta * c0 in fp64 on the operands' device.  With
    beta == 0, c0 does not enter (it may be None, or hold NaN/Inf)."""
    out = alpha * (b.double().transpose(0, 1) @ a.double())
    if beta != 0:
        out = out + beta * c0.double()
    return out


def bound(a: torch.Tensor, b: torch.Tensor, c0, alpha: float, beta: float,
          K: int, extra=0) -> torch.Tensor:
    """Elementwise fp64 bound E on |got - ref64| (see the module text)."""
    p = b.double().abs().transpose(0, 1) @ a.double().abs()
    mag = abs(alpha) * (p + extra)
    if beta != 0:
        mag = mag + abs(beta) * c0.double().abs()
    return (K + 8) * EPS * mag


def baseline_verdict_ops(m: int, n: int, k: int, panel_k: int) -> int:
    """Rounding operations on either side of a residual of the offline
    checksum chain (ops.baseline_ft); baseline_verdict_bounds says how they
    are counted."""
    npanels = -(-k // panel_k)
    return k + max(m, n) + 2 * npanels + 16


def baseline_verdict_bounds(a: torch.Tensor, b: torch.Tensor, c0,
                            alpha: float, beta: float, panel_k: int):
    """Bounds (b_row (M,), b_col (N,)), fp64, on the residuals whose squared
    norms are the verdicts of the offline checksum chain.

    The row residual r_i is the difference of two fp32 quantities that are
    equal in exact arithmetic: the observed row sum of C, sum_j C_ij, and the
    maintained checksum beta * (C0 e)_i + alpha * sum_p (Ap (Bp^T e))_i.

    Observed side: an element of C passes K multiply-adds, and per panel the
    alpha product and the add into the running C (the first panel also
    beta * C0): K + 2 * npanels + 1 roundings; the row sum adds N - 1 more,
    in any order (the slice-wise atomics included).  Maintained side: a
    product A_ik B_jk passes the N - 1 adds of the operand sum (Bp^T e)_k,
    the kp multiply-adds of the gemv, its alpha product and the npanels adds
    into the checksum: fewer than N + K + 2 * npanels; a C0 term passes N
    adds, the beta product and the npanels adds.  The subtraction rounds
    once.  For the column residual M takes N's place.  So either side is
    reached by at most

        ops = K + max(M, N) + 2 * npanels + 16

    roundings (the count above needs + 2; 16 is kept as room for a library
    reduction that pads or splits its sums), each at most 2**-23 relative
    (twice the round-to-nearest unit, which absorbs the second-order terms
    as ops * 2**-24 << 1), on magnitudes that sum to at most

        S_i = sum_j (|alpha| * P_ij + |beta| * |C0_ij|),
        P = |B| |A|^T,

    and |r_i| <= b_i = 2 * ops * 2**-23 * S_i; b_j likewise with the sum
    over i.  Intermediate panels have done fewer operations on smaller
    magnitudes, so the bound of the whole K holds at every verdict."""
    k, m = a.shape
    n = b.shape[1]
    p = b.double().abs().transpose(0, 1) @ a.double().abs()
    mag = abs(alpha) * p
    if beta != 0:
        mag = mag + abs(beta) * c0.double().abs()
    f = 2 * baseline_verdict_ops(m, n, k, panel_k) * EPS
    return f * mag.sum(dim=0), f * mag.sum(dim=1)


def baseline_verdict_clean_limit(bvec: torch.Tensor) -> float:
    """Largest fault-free verdict: sum b^2, times the relative error of the
    fp32 dot product that forms it (len products and len - 1 adds of
    non-negative terms)."""
    return float((bvec * bvec).sum()) * (1 + (bvec.numel() + 1) * EPS)


def baseline_verdict_fault_band(bvec: torch.Tensor, idx: int, delta: float,
                                ops: int):
    """(lo, hi) for the verdict when one element of row (column) `idx` of C
    carries an additive fault delta; ops = baseline_verdict_ops(...).  The
    fault is one more magnitude |delta| carried through the observed side's
    operations (its own add, the later panels' adds, the row sum), so that
    residual is delta + e with |e| <= b_d = b_idx + 2 * ops * 2**-23 *
    |delta|, and every other residual is bounded as in a clean run:

        (|delta| - b_d)^2 <= verdict <= (|delta| + b_d)^2 + sum b^2,

    each side widened by the fp32 dot product's relative error."""
    b_d = float(bvec[idx]) + 2 * ops * EPS * abs(delta)
    dot = (bvec.numel() + 1) * EPS
    lo = max(abs(delta) - b_d, 0.0) ** 2 * (1 - dot)
    hi = ((abs(delta) + b_d) ** 2 + float((bvec * bvec).sum())) * (1 + dot)
    return lo, hi


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, e: torch.Tensor):
    """(max over elements of |got - ref| / e, its index).  A non-finite
    element of `got` counts as an infinite ratio."""
    diff = (got.double() - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / e)
    ratio = torch.where(torch.isfinite(got.double()), ratio,
                        torch.full_like(ratio, float("inf")))
    ratio = torch.where(torch.isnan(ratio),
                        torch.full_like(ratio, float("inf")), ratio)
    flat = int(torch.argmax(ratio))
    idx = tuple(int(x) for x in
                torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.reshape(-1)[flat]), idx


def assert_within(got, ref, e, what: str = "") -> float:
    """Assert |got - ref| <= e elementwise; the message carries the worst
    ratio diff / E and where it is.  Returns the worst ratio."""
    w, idx = worst_ratio(got, ref, e)
    print(f"[errbound] {what}: worst diff/E = {w:.3e} at {idx}")
    assert w <= 1.0, (f"{what}: worst diff/E = {w:.4g} at {idx} "
                      f"(got {float(got[idx]):.9g}, ref {float(ref[idx]):.9g},"
                      f" E {float(e[idx]):.3e})")
    return w
