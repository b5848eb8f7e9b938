"""CPU tests of the ragged stream-K launch's host side: the partition mirror
(ops.ragged_streamk_partition), the layout and error rules on CPU tensors,
the injector predictor's stream-K form, the gate, and a check that the GPU
file's (shape, grid) cases hold every kind of tile ownership."""

import pytest
import torch

import test_gpu_ragged_streamk as gs
from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING, threads
from ft_sgemm_amd.ops.fault_report import predict_injected_events

SK_TIERS = ("large", "huge")


def partition_shapes(tier):
    t = TILING[tier]
    bm, bn = t["bm"], t["bn"]
    return [(bm + 1, bn + 1, 3 * 64 + 5), (2 * bm + 1, bn + 1, 2 * 64 + 5),
            (3, 5, 7), (1, 1, 1), (2 * bm, 3 * bn, 640), (bm, bn, 64)]


@pytest.mark.parametrize("tier", SK_TIERS)
def test_partition_covers_every_unit_once(tier):
    t = TILING[tier]
    for m, n, k in partition_shapes(tier):
        ntm, ntn, upt = -(-m // t["bm"]), -(-n // t["bn"]), -(-k // 64)
        total = ntm * ntn * upt
        for grid in (1, 2, 3, 4, 5, 7, 16, total, total + 3):
            wgs, g = ops.ragged_streamk_partition(tier, m, n, k, grid)
            assert g == min(grid, total) == len(wgs)
            units, sizes = [], []
            for segs in wgs:
                assert segs  # grid <= total: nobody is idle
                n_units = 0
                for tile, bx, by, w_lo, w_hi, kind in segs:
                    assert 0 <= w_lo < w_hi <= upt
                    assert (bx, by) == (tile % ntm, tile // ntm)
                    assert by < ntn
                    units += [tile * upt + w for w in range(w_lo, w_hi)]
                    n_units += w_hi - w_lo
                sizes.append(n_units)
            # contiguous, k fastest, exactly once; balanced to within one
            assert units == list(range(total))
            assert max(sizes) - min(sizes) <= 1
            assert sizes == sorted(sizes, reverse=True)


@pytest.mark.parametrize("tier", SK_TIERS)
def test_partition_kinds(tier):
    for m, n, k in partition_shapes(tier):
        upt = -(-k // 64)
        for grid in (1, 3, 4, 5, 16):
            wgs, _ = ops.ragged_streamk_partition(tier, m, n, k, grid)
            per_tile = {}
            for wg, segs in enumerate(wgs):
                for i, (tile, _, _, w_lo, w_hi, kind) in enumerate(segs):
                    per_tile.setdefault(tile, []).append((wg, w_lo, w_hi,
                                                          kind))
                    # only a workgroup's first segment can start inside a
                    # tile, only its last can end inside one: two slots
                    assert kind != "head" or i == 0
                    assert kind != "tail" or i == len(segs) - 1
            for tile, segs in per_tile.items():
                # the segments tile [0, upt) in workgroup order
                assert segs[0][1] == 0 and segs[-1][2] == upt
                for (_, _, hi, _), (_, lo, _, _) in zip(segs, segs[1:]):
                    assert hi == lo
                wgs_of_tile = [s[0] for s in segs]
                assert wgs_of_tile == list(range(wgs_of_tile[0],
                                                 wgs_of_tile[-1] + 1))
                kinds = [s[3] for s in segs]
                if len(segs) == 1:
                    assert kinds == ["full"]
                else:
                    assert kinds == ["tail"] + ["head"] * (len(segs) - 1)


def test_short_last_unit_and_clamp():
    # K % 64 != 0: the last unit exists and is short
    wgs, g = ops.ragged_streamk_partition("large", 10, 10, 64 + 5, 2)
    assert g == 2
    assert wgs == [[(0, 0, 0, 0, 1, "tail")], [(0, 0, 0, 1, 2, "head")]]
    ev = predict_injected_events("large", 10, 10, 64 + 5, ragged=True,
                                 streamk_grid=2)
    # bkf = 8: the short unit is one panel, [64, 72)
    assert sorted((e.k_begin, e.k_end) for e in ev) == [(0, 64), (64, 72)]
    wgs, g = ops.ragged_streamk_partition("huge", 10, 10, 5, 1000)
    assert g == 1 and wgs == [[(0, 0, 0, 0, 1, "full")]]
    with pytest.raises(ValueError):
        ops.ragged_streamk_partition("medium", 10, 10, 5, 2)
    with pytest.raises(ValueError):
        ops.ragged_streamk_partition("huge", 10, 10, 5, 0)
    with pytest.raises(ValueError):
        ops.ragged_streamk_partition("huge", 10, 0, 5, 2)


@pytest.mark.parametrize("tier", SK_TIERS)
def test_gpu_cases_hold_every_ownership(tier):
    """The GPU file's cases contain a fully-owned tile, a tile split across
    exactly two workgroups, a tile split across three or more with a
    workgroup lying wholly inside it, and a workgroup holding head + full
    tile + tail."""
    full = two = inside = head_full_tail = False
    for (m, n, k), grid in gs.CASES(tier):
        assert k % 64 != 0  # every tile ends in a short unit
        wgs, _ = ops.ragged_streamk_partition(tier, m, n, k, grid)
        owners = {}
        for wg, segs in enumerate(wgs):
            kinds = [s[5] for s in segs]
            full |= "full" in kinds
            head_full_tail |= (kinds[0] == "head" and kinds[-1] == "tail"
                               and "full" in kinds[1:-1])
            for s in segs:
                owners.setdefault(s[0], []).append((wg, len(segs)))
        for tile, own in owners.items():
            two |= len(own) == 2
            # a middle owner with one segment lies wholly inside the tile
            inside |= len(own) >= 3 and any(ns == 1 for _, ns in own[1:-1])
    assert full and two and inside and head_full_tail
    assert len(gs.CASES(tier)) == gs.N_CASES
    assert gs.CASES(tier)[:5] == gs.split_cases(tier)
    assert [c[0] for c in gs.CASES(tier)[5:]] == [(3, 5, 7), (1, 1, 1)]


def test_layout_rules_on_cpu_tensors():
    need = ops.streamk_partials_floats("large", 4)
    assert need == 2 * 4 * 64 * 64
    assert ops.streamk_partials_floats("huge", 3) == 2 * 3 * 256 * 128
    assert ops.ragged_streamk_layout("large", 65, 65, 197, 4) == 4
    assert ops.ragged_streamk_layout("large", 65, 65, 197, 100) == 16
    buf = torch.empty(need + 4)
    assert buf.data_ptr() % 16 == 0
    assert ops.ragged_streamk_layout("large", 65, 65, 197, 4, buf) == 4
    # a clamped grid needs only the clamped grid's slots
    assert ops.ragged_streamk_layout("large", 10, 10, 5, 4,
                                     buf[:2 * 64 * 64]) == 1
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.ragged_streamk_layout("tall", 65, 65, 197, 4)
    with pytest.raises(ValueError, match="must be >= 1"):
        ops.ragged_streamk_layout("large", 65, 65, 197, 0)
    with pytest.raises(ValueError, match="needs"):
        ops.ragged_streamk_layout("large", 65, 65, 197, 4, buf[:need - 1])
    with pytest.raises(ValueError, match="16-byte"):
        ops.ragged_streamk_layout("large", 65, 65, 197, 4, buf[1:1 + need])
    with pytest.raises(ValueError, match="float32"):
        ops.ragged_streamk_layout("large", 65, 65, 197, 4, buf.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.ragged_streamk_layout("large", 65, 65, 197, 4,
                                  torch.empty(2 * need)[::2])
    with pytest.raises(ValueError, match="work units"):
        ops.ragged_streamk_layout("large", 2**21, 2**21, 128, 4)  # 2^31


def test_call_rules_on_cpu_tensors():
    """What the Python entry refuses before it reaches the extension."""
    a, b, c = torch.zeros(197, 65), torch.zeros(197, 65), torch.zeros(65, 65)
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.sgemm_ragged("medium", a, b, c, streamk=4)
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.ft_sgemm_ragged("wide", a, b, c, streamk="auto")
    with pytest.raises(ValueError, match="2-D"):
        ops.sgemm_ragged("large", a[None], b[None], c[None], streamk=4)
    with pytest.raises(TypeError):
        ops.sgemm_ragged_batched("large", a[None], b[None], c[None],
                                 streamk=4)
    with pytest.raises(ValueError, match="streamk must be"):
        ops.sgemm_ragged("large", a, b, c, streamk="always")
    with pytest.raises(ValueError, match="streamk must be"):
        ops.sgemm_ragged("large", a, b, c, streamk=True)
    with pytest.raises(ValueError, match="must be >= 1"):
        ops.sgemm_ragged("large", a, b, c, streamk=-2)
    with pytest.raises(ValueError, match="partials go with"):
        ops.sgemm_ragged("large", a, b, c, partials=torch.empty(8))
    with pytest.raises(ValueError, match="needs"):
        ops.ft_sgemm_ragged("large", a, b, c, streamk=4,
                            partials=torch.empty(8))


@pytest.mark.parametrize("vw", [20, 2, 1])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_predictor_streamk(tier, vw):
    t = TILING[tier]
    bm, bn, bkf = t["bm"], t["bn"], t.get("bkf", t["bk"])
    m, n, k = bm + 1, bn + 1, 3 * 64 + 5
    upt = 4
    stride = max(1, upt // vw)
    for grid in (1, 3, 5, 16):
        wgs, _ = ops.ragged_streamk_partition(tier, m, n, k, grid, True)
        ev = predict_injected_events(tier, m, n, k, vw, ragged=True,
                                     streamk_grid=grid)
        groups = sum(-(-(s[4] - s[3]) // stride) for segs in wgs
                     for s in segs)
        assert len(ev) == groups
        for e in ev:
            assert e.corrected and e.k_begin % 64 == 0
            assert e.k_begin < e.k_end <= 4 * 64
            assert e.k_end % bkf == 0 and e.k_end - e.k_begin <= 64 * stride
            assert 0 <= e.i < 2 * bm and 0 <= e.j < 2 * bn
            assert e.band_rows == t["wm"] and e.i - e.band_row in range(
                0, t["wm"], 4)
        # the groups of one tile cover its K once, whole panels at the end
        per_tile = {}
        for e in ev:
            per_tile.setdefault((e.i // bm, e.j // bn), []).append(
                (e.k_begin, e.k_end))
        assert len(per_tile) == 4
        for spans in per_tile.values():
            spans.sort()
            assert spans[0][0] == 0 and spans[-1][1] == -(-k // bkf) * bkf
            for (_, hi), (lo, _) in zip(spans, spans[1:]):
                assert hi == lo
    # grid = 1, one group per tile: the victim of unit 0 of tile `tile`
    ev = predict_injected_events(tier, m, n, k, 1, ragged=True,
                                 streamk_grid=1)
    assert len(ev) == 4
    tids = sorted((tile * 13) % threads(tier) for tile in range(4))
    waves_n = bn // t["wn"]
    got = sorted(((e.i % bm) // t["wm"] * waves_n + (e.j % bn) // t["wn"]) * 64
                 + ((e.i % bm) % t["wm"] // 4) * 32 + (e.j % bn) % t["wn"]
                 for e in ev)
    assert got == tids
    with pytest.raises(ValueError):
        predict_injected_events(tier, m, n, k, streamk_grid=3)


def test_classic_predictor_unchanged():
    ev = predict_injected_events("large", 65, 65, 197, ragged=True)
    assert ev == predict_injected_events("large", 65, 65, 197, ragged=True,
                                         streamk_grid=0)


def test_gate_and_note():
    for tier in TIERS:
        for shape in ((1024, 1024, 16384), (4097, 4097, 4096), (1, 1, 1)):
            for fused in (False, True):
                g = ops.ragged_streamk_gate(tier, *shape, fused)
                assert isinstance(g, bool)
                if not TILING[tier].get("streamk", False):
                    assert g is False
    assert isinstance(ops.RAGGED_STREAMK_NOTE, str)
    assert "profiles/ragged_streamk.txt" in ops.RAGGED_STREAMK_NOTE


def test_ft_linear_takes_streamk_flag():
    import inspect
    assert inspect.signature(ops.ft_linear).parameters[
        "streamk"].default is False
    assert ops.FTLinear(4, 3, streamk=True).streamk is True
    assert ops.FTLinear(4, 3).streamk is False
