"""CPU tests of the grouped ragged launch's Python side: ops.grouped_layout
(the mirror of grouped_args_error), ops.choose_tier_grouped, the generated
grouped translation units and ft_grouped_linear's argument checks."""

import os

import pytest
import torch

from ft_sgemm_amd import kernel_table as kt
from ft_sgemm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def operands(m, n, k, trans_a=False, trans_b=False):
    a = torch.zeros((m, k) if trans_a else (k, m))
    b = torch.zeros((n, k) if trans_b else (k, n))
    return a, b, torch.zeros((n, m))


def lists(shapes, trans_a=False, trans_b=False):
    return tuple(map(list, zip(*(operands(*s, trans_a, trans_b)
                                 for s in shapes))))


MIXED = [(1, 1, 1), (17, 15, 33), (64, 32, 64), (40, 0, 8), (0, 5, 8),
         (24, 40, 0)]


@pytest.mark.parametrize("trans_a", [False, True])
@pytest.mark.parametrize("trans_b", [False, True])
def test_layout_accepts_mixed_and_empty_entries(trans_a, trans_b):
    a, b, c = lists(MIXED, trans_a, trans_b)
    got = ops.grouped_layout(a, b, c, trans_a, trans_b)
    assert [g[:3] for g in got] == MIXED
    for (m, n, k), (_, _, _, lda, ldb, ldc) in zip(MIXED, got):
        if m and n and k:
            assert (lda, ldb, ldc) == (k if trans_a else m,
                                       k if trans_b else n, m)


def test_layout_accepts_row_strided_views():
    big_a, big_b, big_c = (torch.zeros(40, 50) for _ in range(3))
    a = [big_a[2:35, 3:20], torch.zeros(8, 5)]    # (K=33, M=17), (8, 5)
    b = [big_b[1:34, 7:22], torch.zeros(8, 3)]    # (K=33, N=15), (8, 3)
    c = [big_c[4:19, 9:26], torch.zeros(3, 5)]    # (N=15, M=17), (3, 5)
    got = ops.grouped_layout(a, b, c)
    assert got[0] == (17, 15, 33, 50, 50, 50)
    assert got[1] == (5, 3, 8, 5, 3, 5)
    # c entries carved out of one buffer, one after the other, are disjoint
    buf = torch.zeros(15 * 17 + 7 + 3 * 5)
    c = [buf[:15 * 17].view(15, 17), buf[15 * 17 + 7:].view(3, 5)]
    a, b = [torch.zeros(33, 17), torch.zeros(8, 5)], [torch.zeros(33, 15),
                                                      torch.zeros(8, 3)]
    assert len(ops.grouped_layout(a, b, c)) == 2


def test_layout_rejects_dtype():
    a, b, c = lists([(4, 4, 4), (3, 3, 3)])
    a[1] = a[1].double()
    with pytest.raises(ValueError, match="float32"):
        ops.grouped_layout(a, b, c)


def test_layout_rejects_inner_stride():
    a, b, c = lists([(4, 4, 4), (3, 5, 7)])
    b[1] = torch.zeros(5, 7).t()  # (7, 5) with inner stride 7
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.grouped_layout(a, b, c)


def test_layout_rejects_shape_disagreement():
    a, b, c = lists([(4, 4, 4), (3, 5, 7)])
    b[1] = torch.zeros(8, 5)  # K = 8 against a's 7
    with pytest.raises(ValueError, match="disagree"):
        ops.grouped_layout(a, b, c)
    a, b, c = lists([(4, 4, 4), (3, 5, 7)])
    c[0] = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="disagree"):
        ops.grouped_layout(a, b, c)


def test_layout_rejects_list_length_mismatch():
    a, b, c = lists([(4, 4, 4), (3, 5, 7)])
    with pytest.raises(ValueError, match="entries"):
        ops.grouped_layout(a, b[:1], c)
    with pytest.raises(ValueError, match="empty group"):
        ops.grouped_layout([], [], [])


def test_layout_rejects_overlapping_c():
    """Two entries that alias the same rows of one buffer."""
    a, b, _ = lists([(6, 4, 3), (6, 4, 3)])
    buf = torch.zeros(6, 6)
    c = [buf[0:4], buf[2:6]]  # rows 2 and 3 belong to both
    with pytest.raises(ValueError, match="overlap"):
        ops.grouped_layout(a, b, c)
    with pytest.raises(ValueError, match="overlap"):
        ops.grouped_layout(a, b, [buf[0:4], buf[0:4]])
    # an empty entry writes nothing and may alias anything
    a, b, _ = lists([(6, 4, 3), (6, 0, 3)])
    assert len(ops.grouped_layout(a, b, [buf[0:4], buf[2:2]])) == 2


def test_layout_rejects_c_interleaved_in_a_row():
    """Heads inside a (tokens, heads*dim) tensor: legal for the strided batch,
    not for a grouped launch, whose rule is on address intervals."""
    a, b, _ = lists([(8, 5, 3), (8, 5, 3)])
    wide = torch.zeros(5, 16)
    c = [wide[:, 0:8], wide[:, 8:16]]
    with pytest.raises(ValueError, match="interleaved within a row"):
        ops.grouped_layout(a, b, c)


SHAPE_SETS = [
    [(1, 1, 1)],
    [(0, 0, 0)],
    [(5, 0, 3), (0, 4, 2)],
    [(7, 9, 0)],
    MIXED,
    [(4096, 4096, 64)] * 2,
    [(128, 64, 512)] * 300,
    [(4096, 8, 64)] * 3,
    [(8, 4096, 64)] * 3,
    [(64, 64, 64)] * 1100,
]


@pytest.mark.parametrize("shapes", SHAPE_SETS, ids=range(len(SHAPE_SETS)))
def test_choose_tier_grouped_always_returns_a_tier(shapes):
    assert ops.choose_tier_grouped(shapes) in kt.TIERS
    # the six-field form grouped_layout returns is taken as well
    assert ops.choose_tier_grouped([s + (1, 1, 1) for s in shapes]) == \
        ops.choose_tier_grouped(shapes)


@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 15, 33), (512, 512, 512),
                                   (4097, 4097, 100), (8193, 257, 1025),
                                   (257, 8193, 64), (1000, 1000, 333),
                                   (2048, 2048, 256)])
def test_choose_tier_grouped_single_entry_is_the_ragged_choice(shape):
    assert ops.choose_tier_grouped([shape]) == \
        ops.choose_tier(*shape, ragged=True)


def test_choose_tier_grouped_uses_the_total_tile_count():
    # 2 x 256 huge tiles: neither entry reaches 384 by itself
    one = (4096, 2048, 64)
    assert ops.choose_tier_grouped([one, one]) == "huge"
    assert isinstance(ops.GROUPED_THRESHOLDS_NOTE, str)
    assert "not fitted" in ops.GROUPED_THRESHOLDS_NOTE


def test_generated_grouped_units():
    gen = os.path.join(ROOT, "csrc", "generated")
    flags = {"nn": ("false", "false"), "tn": ("true", "false"),
             "nt": ("false", "true"), "tt": ("true", "true")}
    for tier in kt.TIERS:
        for sfx, (ta, tb) in flags.items():
            path = os.path.join(gen, f"kernel_{tier}_ragged_grouped_{sfx}.hip")
            assert os.path.exists(path), path
            src = open(path).read()
            assert "launch_tier_ragged_grouped<" in src
            assert f"{ta}, {tb}>(g)" in " ".join(src.split())
    # *_hip.hip are by-products of the extension build, not generated units
    grouped = [f for f in os.listdir(gen)
               if "_grouped" in f and not f.endswith("_hip.hip")]
    assert len(grouped) == len(kt.TIERS) * 4
    assert not [f for f in grouped if f.endswith("_batched.hip")]


def test_grouped_linear_rejects_bad_counts():
    x, w = torch.zeros(10, 6), torch.zeros(3, 4, 6)
    with pytest.raises(ValueError, match="sum to 9"):
        ops.ft_grouped_linear(x, w, [4, 0, 5])
    with pytest.raises(ValueError, match="negative"):
        ops.ft_grouped_linear(x, w, [12, -2, 0])
    with pytest.raises(ValueError, match="2 counts for 3 experts"):
        ops.ft_grouped_linear(x, w, [4, 6])
    with pytest.raises(ValueError, match="integer"):
        ops.ft_grouped_linear(x, w, torch.tensor([4.0, 0.0, 6.0]))
    with pytest.raises(ValueError, match="integers"):
        ops.ft_grouped_linear(x, w, [4, 0.5, 5.5])


def test_grouped_linear_rejects_bad_operands():
    x, w = torch.zeros(10, 6), torch.zeros(3, 4, 6)
    with pytest.raises(ValueError, match=r"\(E, out, in\)"):
        ops.ft_grouped_linear(x, w[0], [10])
    with pytest.raises(ValueError, match="x must be"):
        ops.ft_grouped_linear(torch.zeros(10, 5), w, [4, 0, 6])
    with pytest.raises(ValueError, match="bias must be"):
        ops.ft_grouped_linear(x, w, [4, 0, 6], torch.zeros(4))
    with pytest.raises(ValueError, match="float32"):
        ops.ft_grouped_linear(x.double(), w, [4, 0, 6])


def test_grouped_linear_refuses_cuda_counts():
    """The check reads only counts.is_cuda, so it runs without a device."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    x, w = torch.zeros(10, 6), torch.zeros(3, 4, 6)
    counts = torch.tensor([4, 0, 6]).as_subclass(OnDevice)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.ft_grouped_linear(x, w, counts)
