"""CPU tests of the ragged SGEMM's Python layer: operand validation
(ops.ragged_layout), tier choice (ops.choose_tier(..., ragged=True)) and the
injector's prediction on ceil grids (predict_injected_events /
predict_injection_model with ragged=True)."""

import pytest
import torch

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import ERROR_INJECT, TIERS, TILING, threads
from ft_sgemm_amd.ops.fault_report import (predict_injected_events,
                                           predict_injection_model)


def tensors(m, n, k):
    return torch.zeros(k, m), torch.zeros(k, n), torch.zeros(n, m)


def test_layout_packed():
    a, b, c = tensors(5, 7, 3)
    assert ops.ragged_layout(a, b, c) == (5, 7, 3, 5, 7, 5)


def test_layout_row_strided_views():
    big_a, big_b, big_c = (torch.zeros(9, 20), torch.zeros(9, 30),
                           torch.zeros(12, 25))
    a, b, c = big_a[2:5, 3:8], big_b[2:5, 1:8], big_c[4:11, 6:11]
    assert ops.ragged_layout(a, b, c) == (5, 7, 3, 20, 30, 25)


def test_layout_one_row_uses_width():
    # K == 1: a and b have one row, whose stride says nothing
    a = torch.zeros(4, 20)[1:2, 3:8]
    b = torch.zeros(4, 30)[2:3, 0:7]
    c = torch.zeros(7, 5)
    assert ops.ragged_layout(a, b, c) == (5, 7, 1, 5, 7, 5)
    # N == 1: c has one row
    a, b = torch.zeros(3, 5), torch.zeros(3, 1)
    c = torch.zeros(2, 40)[1:2, 0:5]
    assert ops.ragged_layout(a, b, c) == (5, 1, 3, 5, 1, 5)


def test_layout_rejects():
    a, b, c = tensors(6, 8, 4)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.ragged_layout(torch.zeros(4, 12)[:, ::2], b, c)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.ragged_layout(a, b, torch.zeros(6, 8).t())
    with pytest.raises(ValueError, match="float32"):
        ops.ragged_layout(a.double(), b, c)
    with pytest.raises(ValueError, match="disagree"):
        ops.ragged_layout(a, torch.zeros(5, 8), c)
    with pytest.raises(ValueError, match="disagree"):
        ops.ragged_layout(a, b, torch.zeros(6, 8))
    with pytest.raises(ValueError, match="2-D"):
        ops.ragged_layout(a.unsqueeze(0), b, c)
    with pytest.raises(ValueError, match="overlap"):
        ops.ragged_layout(a, b, torch.zeros(6).expand(8, 6))
    with pytest.raises(ValueError, match="overlap"):
        ops.ragged_layout(a, b, torch.zeros(64).as_strided((8, 6), (5, 1)))
    with pytest.raises(ValueError, match="empty"):
        ops.ragged_layout(*tensors(0, 8, 4))


ODD = [1, 3, 17, 100, 257, 333, 1000, 2049, 4097, 8200]


def test_choose_tier_ragged_never_none():
    for m in ODD:
        for n in ODD:
            for k in (1, 7, 65, 333):
                assert ops.choose_tier(m, n, k, ragged=True) in TIERS


def test_choose_tier_ragged_agrees_where_a_tier_fits():
    sizes = [16, 32, 64, 96, 128, 256, 1024, 2048, 4096, 4160, 6144]
    seen = 0
    for m in sizes + ODD:
        for n in sizes + ODD:
            for k in (16, 32, 64, 333):
                want = ops.choose_tier(m, n, k)
                if want is not None:
                    seen += 1
                    assert ops.choose_tier(m, n, k, ragged=True) == want
    assert seen > 100


def test_choose_tier_ragged_uses_ceil_tile_counts():
    # 4097^2: 17 x 33 = 561 huge tiles >= 384
    assert ops.choose_tier(4097, 4097, 4097, ragged=True) == "huge"
    # skinny shapes keep their tier
    assert ops.choose_tier(4097, 100, 333, ragged=True) == "tall"
    assert ops.choose_tier(100, 4097, 333, ragged=True) == "wide"
    # 2049^2: 9 x 17 huge tiles < 384, 33 x 33 = 1089 large tiles >= 1024
    assert ops.choose_tier(2049, 2049, 100, ragged=True) == "large"
    assert ops.choose_tier(100, 100, 100, ragged=True) == "medium"
    with pytest.raises(ValueError):
        ops.choose_tier(100, 100, 100, batch=2, ragged=True)
    assert "not measured" in ops.RAGGED_THRESHOLDS_NOTE


def geom(tier):
    t = TILING[tier]
    return t["bm"], t["bn"], t.get("bkf", t["bk"]), t["wm"], t["wn"]


@pytest.mark.parametrize("tier", TIERS)
def test_prediction_equals_tiled_on_a_divisible_shape(tier):
    bm, bn, bkf, _, _ = geom(tier)
    m, n, k = 2 * bm, 3 * bn, 256
    assert (predict_injected_events(tier, m, n, k, ragged=True) ==
            predict_injected_events(tier, m, n, k))
    a = predict_injection_model(tier, m, n, k, 9500.0, ERROR_INJECT)
    b = predict_injection_model(tier, m, n, k, 9500.0, ERROR_INJECT,
                                ragged=True)
    assert torch.equal(a.mult, b.mult) and torch.equal(a.residue, b.residue)
    assert a[2:7] == b[2:7]
    assert a.wave_totals == b.wave_totals and a.col_totals == b.col_totals


@pytest.mark.parametrize("tier", TIERS)
def test_prediction_on_an_edge_shape(tier):
    bm, bn, bkf, wm, wn = geom(tier)
    m, n, k = bm + 1, bn + 1, 6 * bkf + 5
    with pytest.raises(ValueError):
        predict_injected_events(tier, m, n, k)
    ev = predict_injected_events(tier, m, n, k, ragged=True)
    # 2 x 2 blocks, ceil(k / bkf) = 7 panels, one window each
    assert len(ev) == 4 * 7
    assert any(e.i >= m or e.j >= n for e in ev), "padded victims expected"
    assert {(e.k_begin, e.k_end) for e in ev} == {
        (w * bkf, (w + 1) * bkf) for w in range(7)}
    assert max(e.k_end for e in ev) == 7 * bkf > k
    # the rule itself, block (1, 1), window 3
    tid = (3 * 67) % threads(tier)
    wave, lane = tid >> 6, tid & 63
    mm = 16 if TILING[tier]["mfma"] == "f32_16x16x4" else 32
    i = bm + (wave // (bn // wn)) * wm + 4 * (lane // mm)
    j = bn + (wave % (bn // wn)) * wn + lane % mm
    assert any((e.i, e.j, e.k_begin) == (i, j, 3 * bkf) for e in ev)
    mod = predict_injection_model(tier, m, n, k, 9500.0, ERROR_INJECT,
                                  ragged=True)
    assert tuple(mod.mult.shape) == (m, n)
    assert mod.corrected == mod.n_faults == 28 and mod.uncorrected == 0
    assert int(mod.mult.sum()) == sum(e.i < m and e.j < n for e in ev)
    assert float(mod.residue.abs().max()) == 0.0


def test_auto_rejects_an_unknown_misfit():
    a, b, c = tensors(100, 100, 100)
    with pytest.raises(ValueError, match="misfit"):
        ops.ft_sgemm_auto(a, b, c, misfit="pad")
