"""CPU tests of the grouped stream-K launch's host side: the partition mirror
(ops.grouped_streamk_partition), the layout rules on CPU tensors, the grouped
injector predictor, the gate, and a check that the GPU file's group and grids
hold every kind of ownership the kernel's walk has."""

import inspect
import random

import pytest
import torch

import test_gpu_grouped_streamk as gg
from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING
from ft_sgemm_amd.ops.fault_report import (predict_injected_events,
                                           predict_injected_events_grouped)

SK_TIERS = ("large", "huge")


def random_groups(tier, seed, count=40):
    """Seeded shape lists with empty entries of every kind, K tails and
    entries of several tiles."""
    t = TILING[tier]
    rng = random.Random(seed)
    sizes_m = [0, 1, 3, t["bm"] - 1, t["bm"], t["bm"] + 1, 2 * t["bm"] + 1]
    sizes_n = [0, 1, 5, t["bn"] - 1, t["bn"], t["bn"] + 1, 2 * t["bn"] + 1]
    sizes_k = [0, 1, 7, 63, 64, 65, 128, 3 * 64 + 5, 640]
    out = []
    for _ in range(count):
        out.append([(rng.choice(sizes_m), rng.choice(sizes_n),
                     rng.choice(sizes_k))
                    for _ in range(rng.randint(1, 7))])
    return out


def unit_list(tier, shapes):
    """Every unit (entry, tile, w) in the kernel's order."""
    out = []
    for e, (ntm, ntn, upt) in enumerate(
            ops.grouped_streamk_units(tier, shapes)):
        out += [(e, tile, w) for tile in range(ntm * ntn)
                for w in range(upt)]
    return out


@pytest.mark.parametrize("tier", SK_TIERS)
def test_partition_properties(tier):
    for shapes in random_groups(tier, 11) + [gg.group(tier)]:
        want = unit_list(tier, shapes)
        units = ops.grouped_streamk_units(tier, shapes)
        for grid in (1, 2, 3, 5, 7, 16, len(want) + 3):
            wgs, g = ops.grouped_streamk_partition(tier, shapes, grid)
            if not want:
                assert (wgs, g) == ([], 0)
                continue
            assert g == min(grid, len(want)) and len(wgs) == g
            # covers every unit exactly once, contiguously, in order
            got = [(e, tile, w) for segs in wgs
                   for e, tile, _, _, w_lo, w_hi, _ in segs
                   for w in range(w_lo, w_hi)]
            assert got == want
            # balanced to within one unit, the long ranges first
            sizes = [sum(s[5] - s[4] for s in segs) for segs in wgs]
            assert max(sizes) - min(sizes) <= 1
            assert sizes == sorted(sizes, reverse=True)
            per_tile = {}
            for wg, segs in enumerate(wgs):
                kinds = [s[6] for s in segs]
                assert kinds.count("head") <= 1 and kinds.count("tail") <= 1
                for i, (e, tile, bx, by, w_lo, w_hi, kind) in enumerate(segs):
                    ntm, ntn, upt = units[e]
                    assert tile == bx + by * ntm and bx < ntm and by < ntn
                    assert 0 <= w_lo < w_hi <= upt
                    assert kind == ("full" if (w_lo, w_hi) == (0, upt)
                                    else "tail" if w_lo == 0 else "head")
                    # only a workgroup's first segment can start inside a
                    # tile, only its last can end inside one: two slots
                    assert kind != "head" or i == 0
                    assert kind != "tail" or i == len(segs) - 1
                    per_tile.setdefault((e, tile), []).append((wg, kind))
            # a tile is one full, or one tail then heads in workgroup order
            for owners in per_tile.values():
                kinds = [k for _, k in owners]
                if len(owners) == 1:
                    assert kinds == ["full"]
                else:
                    assert kinds == ["tail"] + ["head"] * (len(owners) - 1)
                    wg_ids = [w for w, _ in owners]
                    assert wg_ids == list(range(wg_ids[0],
                                                wg_ids[0] + len(owners)))


@pytest.mark.parametrize("tier", SK_TIERS)
def test_single_entry_is_the_single_launch(tier):
    t = TILING[tier]
    for m, n, k in ((t["bm"] + 1, t["bn"] + 1, 197), (3, 5, 7), (1, 1, 1),
                    (2 * t["bm"], 3 * t["bn"], 640)):
        for grid in (1, 3, 5, 16):
            wgs, g = ops.grouped_streamk_partition(tier, [(m, n, k)], grid)
            ref, g_ref = ops.ragged_streamk_partition(tier, m, n, k, grid)
            assert g == g_ref
            assert [[s[1:] for s in segs] for segs in wgs] == ref
            assert all(s[0] == 0 for segs in wgs for s in segs)


def test_k_zero_and_empty_entries():
    # an entry with k == 0 has one empty unit per tile; m == 0 or n == 0 none
    assert ops.grouped_streamk_units("large", [(65, 65, 0), (0, 5, 9),
                                               (5, 0, 9), (1, 1, 64)]) == \
        [(2, 2, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
    wgs, g = ops.grouped_streamk_partition(
        "large", [(65, 65, 0), (0, 5, 9), (1, 1, 64)], 2)
    assert g == 2
    assert wgs[0] == [(0, 0, 0, 0, 0, 1, "full"), (0, 1, 1, 0, 0, 1, "full"),
                      (0, 2, 0, 1, 0, 1, "full")]
    assert wgs[1] == [(0, 3, 1, 1, 0, 1, "full"), (2, 0, 0, 0, 0, 1, "full")]
    assert ops.grouped_streamk_partition("large", [(0, 5, 9)], 4) == ([], 0)
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.grouped_streamk_partition("medium", [(5, 5, 9)], 4)
    with pytest.raises(ValueError, match=">= 1"):
        ops.grouped_streamk_partition("large", [(5, 5, 9)], 0)


@pytest.mark.parametrize("tier", SK_TIERS)
def test_gpu_group_holds_every_ownership(tier):
    """The GPU file's group and grids contain a fully-owned tile, a tile
    split over two workgroups, one split over three or more with a workgroup
    wholly inside it, a workgroup with head + full + tail, a workgroup whose
    range crosses an entry boundary, a K == 0 tile at the start and one in
    the middle of a workgroup's range, and an empty entry between two live
    ones."""
    bm, bn = TILING[tier]["bm"], TILING[tier]["bn"]
    shapes = gg.group(tier)
    assert shapes == [(bm + 1, bn + 1, 3 * 64 + 5), (3, 5, 7), (0, 5, 9),
                      (bm, bn, 0), (2 * bm + 1, bn + 1, 2 * 64 + 5),
                      (1, 1, 1)]
    total = len(unit_list(tier, shapes))
    assert set(gg.GRIDS) >= {1, 3, 5, 7, 16} and max(gg.GRIDS) > total
    # an empty entry between two live ones
    live = [min(s[:2]) > 0 for s in shapes]
    assert any(live[i - 1] and not live[i] and live[i + 1]
               for i in range(1, len(shapes) - 1))
    full = two = inside = hft = cross = kz_start = kz_mid = False
    for grid in gg.GRIDS:
        wgs, _ = ops.grouped_streamk_partition(tier, shapes, grid)
        per_tile = {}
        for wg, segs in enumerate(wgs):
            kinds = [s[6] for s in segs]
            full |= "full" in kinds
            hft |= (kinds[0] == "head" and kinds[-1] == "tail" and
                    "full" in kinds[1:-1])
            cross |= len({s[0] for s in segs}) > 1
            kz = [i for i, s in enumerate(segs) if shapes[s[0]][2] == 0]
            kz_start |= 0 in kz and len(segs) > 1
            kz_mid |= any(0 < i < len(segs) - 1 for i in kz)
            for s in segs:
                per_tile.setdefault(s[:2], []).append((wg, len(segs)))
        for owners in per_tile.values():
            two |= len(owners) == 2
            # a middle owner with one segment lies wholly inside the tile
            inside |= len(owners) >= 3 and any(ns == 1
                                               for _, ns in owners[1:-1])
    assert full and two and inside and hft
    assert cross and kz_start and kz_mid


def test_layout_rules_on_cpu_tensors():
    shapes = gg.group("large")
    total = len(unit_list("large", shapes))
    assert ops.grouped_streamk_layout("large", shapes, 5) == 5
    assert ops.grouped_streamk_layout("large", shapes, total + 9) == total
    assert ops.grouped_streamk_layout("large", [(0, 5, 9)], 4) == 0
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.grouped_streamk_layout("medium", shapes, 4)
    for grid in (0, -1):
        with pytest.raises(ValueError, match=">= 1"):
            ops.grouped_streamk_layout("large", shapes, grid)
    need = ops.streamk_partials_floats("large", 4)
    buf = torch.zeros(need + 4)
    assert buf.data_ptr() % 16 == 0
    assert ops.grouped_streamk_layout("large", shapes, 4, buf[:need]) == 4
    with pytest.raises(ValueError, match="needs"):
        ops.grouped_streamk_layout("large", shapes, 4, buf[:need - 1])
    with pytest.raises(ValueError, match="16-byte"):
        ops.grouped_streamk_layout("large", shapes, 4, buf[1:1 + need])
    with pytest.raises(ValueError, match="contiguous"):
        ops.grouped_streamk_layout("large", shapes, 4,
                                   torch.zeros(2 * need)[::2])
    with pytest.raises(ValueError, match="float32"):
        ops.grouped_streamk_layout("large", shapes, 4,
                                   torch.zeros(need, dtype=torch.float64))
    # a grid beyond the units is clamped before the partials are sized
    one = ops.streamk_partials_floats("large", 1)
    assert ops.grouped_streamk_layout("large", [(1, 1, 1)], 9,
                                      torch.zeros(one)) == 1
    with pytest.raises(ValueError, match="2\\^31"):
        ops.grouped_streamk_layout("large", [(64 * 4096, 64 * 4096, 64 * 200)],
                                   4)


def test_plan_rules_on_cpu_tensors():
    """What GroupedPlan refuses before it reaches the extension."""
    a, b, c = [torch.zeros(197, 65)], [torch.zeros(197, 65)], \
        [torch.zeros(65, 65)]
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.GroupedPlan("medium", a, b, c, streamk=4)
    with pytest.raises(ValueError, match="no stream-K twin"):
        ops.GroupedPlan("medium", a, b, c, streamk="auto")
    for bad in (-1, True, 2.0, "yes"):
        with pytest.raises(ValueError, match="streamk must be"):
            ops.GroupedPlan("large", a, b, c, streamk=bad)
    with pytest.raises(ValueError, match="partials go with"):
        ops.GroupedPlan("large", a, b, c, partials=torch.zeros(8))
    with pytest.raises(ValueError, match="needs"):
        ops.sgemm_grouped("large", a, b, c, streamk=4,
                          partials=torch.zeros(8))
    with pytest.raises(ValueError, match="streamk must be"):
        ops.ft_grouped_linear(torch.zeros(4, 8), torch.zeros(2, 8, 8),
                              [2, 2], streamk="auto")
    for fn in (ops.sgemm_grouped, ops.ft_sgemm_grouped):
        p = inspect.signature(fn).parameters
        assert p["streamk"].default == 0 and p["partials"].default is None
    assert inspect.signature(ops.ft_grouped_linear).parameters[
        "streamk"].default is False


@pytest.mark.parametrize("vw", [20, 2])
@pytest.mark.parametrize("tier", SK_TIERS)
def test_predictor_grouped(tier, vw):
    t = TILING[tier]
    m, n, k = t["bm"] + 1, t["bn"] + 1, 3 * 64 + 5
    for grid in (1, 3, 5, 16):
        assert predict_injected_events_grouped(
            tier, [(m, n, k)], vw, grid) == [predict_injected_events(
                tier, m, n, k, vw, ragged=True, streamk_grid=grid)]
    # the classic form: every entry its own ragged launch, empty ones none
    shapes = gg.group(tier)
    ev = predict_injected_events_grouped(tier, shapes, vw)
    assert ev[2] == [] and ev[3] == []
    assert ev[1] == predict_injected_events(tier, 3, 5, 7, vw, ragged=True)
    # stream-K: empty and K == 0 entries have no events; every segment with
    # panels has at least one, and the per-entry strides are the entries' own
    for grid in gg.GRIDS:
        ev = predict_injected_events_grouped(tier, shapes, vw, grid)
        assert len(ev) == len(shapes) and ev[2] == [] and ev[3] == []
        wgs, _ = ops.grouped_streamk_partition(tier, shapes, grid)
        for e, (mm, nn, kk) in enumerate(shapes):
            if kk == 0 or mm == 0 or nn == 0:
                continue
            stride = max(1, -(-kk // 64) // vw)
            want = sum(-(-(s[5] - s[4]) // stride)
                       for segs in wgs for s in segs if s[0] == e)
            assert len(ev[e]) == want
            assert all(0 <= x.k_begin < x.k_end for x in ev[e])


def test_gate_and_note():
    small = [(72, 40, 70), (72, 40, 0), (72, 40, 5), (72, 40, 130)]
    for tier in TIERS:
        for fused in (False, True):
            got = ops.grouped_streamk_gate(tier, small, fused)
            assert got is False
            if tier not in SK_TIERS:
                assert ops.grouped_streamk_gate(
                    tier, [(1024, 1024, 8192)] * 8, fused) is False
    # the measured cells of profiles/grouped_streamk.txt, grad_weight at
    # in = out = 1024: halving counts won on both tiers, 8 x 8192 on huge
    # alone, 8 x 512 and the forward products nowhere
    halving = [2048, 1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 2, 0, 0, 0, 0]
    for fused in (False, True):
        for counts, huge, large in ((halving, True, True),
                                    ([8192] * 8, True, False),
                                    ([512] * 8, False, False)):
            gw = [(1024, 1024, n) for n in counts]
            assert ops.grouped_streamk_gate("huge", gw, fused) is huge
            assert ops.grouped_streamk_gate("large", gw, fused) is large
            fwd = [(1024, n, 1024) for n in counts]
            assert ops.grouped_streamk_gate("huge", fwd, fused) is False
            assert ops.grouped_streamk_gate("large", fwd, fused) is False
    assert isinstance(ops.GROUPED_STREAMK_NOTE, str)
    assert "measured" in ops.GROUPED_STREAMK_NOTE
