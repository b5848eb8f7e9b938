"""CPU tests around the offline checksum chain's detection: the raise logic
of ops.ft_sgemm_auto's fallback, and the derived verdict bound of
tests/test_gpu_baseline_detect.py held against an fp32 emulation of the
chain (ops.golden.baseline_ft_emulate) at every shape the GPU tests use."""

import math

import numpy as np
import pytest
import torch

import test_gpu_baseline_detect as gd
from ft_sgemm_amd import ops
from ft_sgemm_amd.ops import golden
from ft_sgemm_amd.utils import errbound as eb

NAN, INF = float("nan"), float("inf")


def misfit():
    m, n, k = 100, 100, 100
    assert ops.choose_tier(m, n, k) is None
    return torch.zeros(k, m), torch.zeros(k, n), torch.zeros(n, m)


@pytest.mark.parametrize("verdict", [(NAN, 0.0), (0.0, NAN), (INF, 0.0),
                                     (0.0, INF), (NAN, NAN), (0.0, 1e9),
                                     (1e9, 0.0)], ids=str)
def test_auto_raises_on_a_bad_verdict(verdict, monkeypatch):
    a, b, c = misfit()
    monkeypatch.setattr(ops, "baseline_ft",
                        lambda a, b, c, *args, **kw: (c, verdict))
    with pytest.raises(RuntimeError, match="offline ABFT verdict"):
        ops.ft_sgemm_auto(a, b, c)


def test_auto_returns_c_on_a_clean_verdict(monkeypatch):
    a, b, c = misfit()
    monkeypatch.setattr(ops, "baseline_ft",
                        lambda a, b, c, *args, **kw: (c, (1e-3, 1e-3)))
    assert ops.ft_sgemm_auto(a, b, c) is c


def cpu_case(shape, panel_k):
    a, b, c0 = gd.operands(*shape, "cpu")
    cs = gd.bounds(a, b, c0, panel_k)  # asserts sum b^2 <= 200^2 / 100
    # the emulation's layout: A (M, K), B (N, K), C0 (M, N)
    cs.np = (a.numpy().T, b.numpy().T, c0.numpy().T)
    return cs


ALL_CASES = ([(s, s[2]) for s in gd.SHAPES] +
             [(gd.CADENCE_SHAPE, gd.CADENCE_PANEL_K),
              (gd.NONFINITE_SHAPE, gd.NONFINITE_PANEL_K), ((257, 129, 65), 32)])


@pytest.mark.parametrize("shape,panel_k", ALL_CASES, ids=str)
def test_emulated_clean_residuals_sit_inside_the_bound(shape, panel_k):
    cs = cpu_case(shape, panel_k)
    _, panels = golden.baseline_ft_emulate(*cs.np, gd.ALPHA, gd.BETA, panel_k,
                                           verify_every=1)
    assert [p for p, _, _ in panels] == list(range(-(-shape[2] // panel_k)))
    worst_r = worst_c = 0.0
    for _, rr, rc in panels:
        worst_r = max(worst_r, float((np.abs(rr) / cs.b_row.numpy()).max()))
        worst_c = max(worst_c, float((np.abs(rc) / cs.b_col.numpy()).max()))
        assert float(rr @ rr) <= cs.lim_row and float(rc @ rc) <= cs.lim_col
    print(f"[baseline-bound] {shape} panel_k {panel_k}: ops {cs.ops}, "
          f"sum b^2 row {cs.lim_row:.4g} col {cs.lim_col:.4g}, emulated "
          f"worst |r|/b row {worst_r:.2e} col {worst_c:.2e}")
    assert worst_r <= 1.0 and worst_c <= 1.0


@pytest.mark.parametrize("delta", [gd.MAG_SMALL, gd.MAG_BIG])
@pytest.mark.parametrize("shape,panel_k", ALL_CASES, ids=str)
def test_emulated_fault_sits_inside_the_band(shape, panel_k, delta):
    cs = cpu_case(shape, panel_k)
    i, j = shape[0] - 1, shape[1] // 2
    _, panels = golden.baseline_ft_emulate(
        *cs.np, gd.ALPHA, gd.BETA, panel_k, verify_every=1,
        fault=(0, i, j, delta, False))
    for _, rr, rc in panels:
        lo, hi = eb.baseline_verdict_fault_band(cs.b_row, i, delta, cs.ops)
        assert lo <= float(rr @ rr) <= hi
        lo, hi = eb.baseline_verdict_fault_band(cs.b_col, j, delta, cs.ops)
        assert lo <= float(rc @ rc) <= hi
        # a band, not a blanket: a fault of half the size falls out of it
        assert hi < (1.5 * delta) ** 2 and lo > (0.75 * delta) ** 2


def test_emulated_nan_fault_gives_nan_verdicts():
    cs = cpu_case(gd.NONFINITE_SHAPE, gd.NONFINITE_PANEL_K)
    i, j = gd.NONFINITE_SITE
    _, panels = golden.baseline_ft_emulate(
        *cs.np, gd.ALPHA, gd.BETA, gd.NONFINITE_PANEL_K,
        fault=(0, i, j, NAN, True))
    assert [p for p, _, _ in panels] == [1, 2]
    for _, rr, rc in panels:
        assert math.isnan(float(rr @ rr)) and math.isnan(float(rc @ rc))


def test_sites_cover_each_reduction_path():
    """The site list reaches what it is there for: band 2 and slice 2 at
    the big shapes, the last f32x4 row, and nothing out of range."""
    assert (1024, 64) in gd.sites(1028, 132) and (1024, 64) in gd.sites(1030, 65)
    assert (1027, 66) in gd.sites(1028, 132) and (1027, 32) in gd.sites(1030, 65)
    assert gd.sites(1, 1) == [(0, 0)]
    for m, n, _ in gd.SHAPES:
        assert all(0 <= i < m and 0 <= j < n for i, j in gd.sites(m, n))
