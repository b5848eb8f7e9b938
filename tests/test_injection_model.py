"""predict_injection_model, the CPU model that tests/test_gpu_threshold.py
holds the device to: the injector's rotation followed through the verify
threshold.  Checked here against predict_injected_events (same rotation
rule) and against cases worked out by hand."""

import pytest
import torch

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING, threads

K = 256
TAU = 9500.0


def _shape(tier):
    return 2 * TILING[tier]["bm"], TILING[tier]["bn"]


@pytest.mark.parametrize("inj", [10000.0, -10000.0, 1.05 * TAU])
@pytest.mark.parametrize("tier", TIERS)
def test_over_tau_every_injection_is_one_corrected_event(tier, inj):
    m, n = _shape(tier)
    ev = ops.predict_injected_events(tier, m, n, K)
    mod = ops.predict_injection_model(tier, m, n, K, TAU, inj)
    assert mod.tripped == mod.corrected == mod.n_faults == len(ev)
    assert (mod.uncorrected, mod.unlocated) == (0, 0)
    want = torch.zeros((m, n), dtype=torch.int32)
    for e in ev:
        want[e.i, e.j] += 1
    assert torch.equal(mod.mult, want)
    assert int(mod.mult.max()) == 1  # no site repeats
    assert not mod.residue.any()
    assert max(mod.wave_totals.values()) == abs(inj)
    assert max(mod.col_totals.values()) == abs(inj)


@pytest.mark.parametrize("tier", TIERS)
def test_small_faults_stay_and_trip_nothing(tier):
    m, n = _shape(tier)
    mod = ops.predict_injection_model(tier, m, n, K, TAU, 200.0)
    assert max(mod.wave_totals.values()) < TAU
    assert (mod.tripped, mod.corrected, mod.uncorrected, mod.unlocated,
            mod.n_faults) == (0, 0, 0, 0, 0)
    assert torch.equal(mod.residue, 200.0 * mod.mult.double())
    ev = ops.predict_injected_events(tier, m, n, K)
    assert int(mod.mult.sum()) == len(ev)
    # per wave the peak total is 200 x the injections that wave received
    t = TILING[tier]
    for (bx, by, wv), tot in mod.wave_totals.items():
        waves_n = t["bn"] // t["wn"]
        i0 = bx * t["bm"] + (wv // waves_n) * t["wm"]
        j0 = by * t["bn"] + (wv % waves_n) * t["wn"]
        cnt = int(mod.mult[i0:i0 + t["wm"], j0:j0 + t["wn"]].sum())
        assert tot == 200.0 * cnt


def test_huge_faults_that_add_up():
    """huge, K = 256: 16 windows, window w goes to wave w % 4.  At 4000 per
    fault a wave's total passes 9500 with its third fault — wave 0 at window
    8, wave 1 at 9, wave 2 at 10, wave 3 at 11 — and, nothing being
    corrected, trips at every later window too: 8 + 7 + 6 + 5 per block."""
    m, n = _shape("huge")
    mod = ops.predict_injection_model("huge", m, n, K, TAU, 4000.0)
    assert max(mod.col_totals.values()) == 4000.0
    assert mod.tripped == mod.unlocated == 2 * 26
    assert (mod.corrected, mod.uncorrected, mod.n_faults) == (0, 0, 0)
    assert torch.equal(mod.residue, 4000.0 * mod.mult.double())
    assert all(v == 16000.0 for v in mod.wave_totals.values())


@pytest.mark.parametrize("tier", TIERS)
def test_faults_that_add_up_every_tier(tier):
    m, n = _shape(tier)
    mod = ops.predict_injection_model(tier, m, n, K, TAU, 4000.0)
    assert max(mod.col_totals.values()) <= TAU
    assert mod.tripped == mod.unlocated > 0
    assert mod.n_faults == 0
    assert torch.equal(mod.residue, 4000.0 * mod.mult.double())


def test_same_column_faults_blend():
    """Two under-tau faults in one column whose sum passes tau: the ratio
    locate blends their rows.  small tier, 1000 windows asked at K = 2048
    (64 windows, one wave of 64 lanes, 16 columns): lanes 0 and 48 share
    column 0 at rows 0 and 12."""
    tier = "small"
    mod = ops.predict_injection_model(tier, 16, 16, 2048, TAU, 5000.0,
                                      verify_windows=1000)
    # every lane is hit exactly once: rows 0, 4, 8, 12 of every column
    assert int(mod.mult.sum()) == 64 == threads(tier)
    assert mod.corrected > 0 and mod.unlocated > 0
    # the blended corrections leave magnitude behind: not a clean result
    assert mod.residue.abs().max() > 0


@pytest.mark.parametrize("vw,k,tier,nwin", [
    (1, 256, "huge", 1), (7, 256, "huge", 8), (1000, 256, "huge", 16),
    (1, 208, "huge", 1), (7, 208, "huge", 13), (1000, 208, "huge", 13),
    (1, 256, "small", 1), (7, 256, "small", 8), (1000, 256, "small", 8),
])
def test_verify_windows(vw, k, tier, nwin):
    m, n = _shape(tier)
    assert nwin <= threads(tier)
    ev = ops.predict_injected_events(tier, m, n, k, verify_windows=vw)
    mod = ops.predict_injection_model(tier, m, n, k, TAU, 1e4,
                                      verify_windows=vw)
    assert len(ev) == 2 * nwin == mod.n_faults == mod.corrected
    assert int(mod.mult.max()) == 1


def test_rejects_undivided_shape():
    with pytest.raises(ValueError):
        ops.predict_injection_model("huge", 100, 128, K, TAU, 1e4)
