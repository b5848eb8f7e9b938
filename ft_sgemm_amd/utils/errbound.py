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
