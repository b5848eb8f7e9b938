"""CPU tests of the strided-batched ragged SGEMM's host-side rules: the
operand layout check (ops.ragged_batched_layout), the tier choice
(ops.choose_tier_ragged_batched) and ops.ft_bmm's argument checks.  Nothing
here touches the extension.
"""

import pytest
import torch

from ft_sgemm_amd import ops

ODD = [1, 3, 17, 100, 257, 333, 1000, 2049, 4097, 8200]  # test_ragged_cpu.py


def tensors(batch, m, n, k):
    return (torch.zeros(batch, k, m), torch.zeros(batch, k, n),
            torch.zeros(batch, n, m))


def test_layout_packed():
    a, b, c = tensors(3, 5, 7, 9)
    assert ops.ragged_batched_layout(a, b, c) == (3, 5, 7, 9, 5, 7, 5,
                                                  45, 63, 35)


def test_layout_row_strided_views():
    big_a, big_b, big_c = (torch.zeros(3, 9, 20), torch.zeros(3, 9, 30),
                           torch.zeros(3, 12, 25))
    a, b, c = big_a[:, 2:6, 3:9], big_b[:, 1:5, 5:13], big_c[:, 4:12, 7:13]
    assert ops.ragged_batched_layout(a, b, c) == (
        3, 6, 8, 4, 20, 30, 25, 180, 270, 300)


def padded(batch, rows, width, gap, ld=None):
    """(batch, rows, width) view with row stride ld and `gap` floats between
    entries."""
    ld = ld or width
    stride = rows * ld + gap
    return torch.zeros(batch * stride).as_strided(
        (batch, rows, width), (stride, ld, 1))


def test_layout_padded_and_odd_batch_strides():
    m, n, k = 5, 7, 9
    a, b, c = padded(3, k, m, 5), padded(3, k, n, 2), padded(3, n, m, 2)
    assert ops.ragged_batched_layout(a, b, c) == (
        3, m, n, k, m, n, m, k * m + 5, k * n + 2, n * m + 2)
    # 50, 65 and 37 floats: none a multiple of 4, two of them odd
    assert all(s % 4 for s in (k * m + 5, k * n + 2, n * m + 2))
    # leading dimension of width + 3 and a gap of 5: odd strides everywhere
    a = padded(3, k, m, 5, m + 3)
    c = padded(3, n, m, 5, m + 3)
    got = ops.ragged_batched_layout(a, b, c)
    assert got[4:] == (m + 3, n, m + 3, k * (m + 3) + 5, k * n + 2,
                       n * (m + 3) + 5)


def test_layout_shared_operands():
    a, b, c = tensors(4, 6, 8, 10)
    a2 = a[0]
    for shared in (a2, a2.unsqueeze(0).expand(4, -1, -1)):
        got = ops.ragged_batched_layout(shared, b, c)
        assert got[:4] == (4, 6, 8, 10) and got[7:] == (0, 80, 48)
    got = ops.ragged_batched_layout(a, b[1], c)
    assert got[7:] == (60, 0, 48)
    # a shared transposed a
    got = ops.ragged_batched_layout(a2.t().contiguous(), b, c, trans_a=True)
    assert got[:8] == (4, 6, 8, 10, 10, 8, 6, 0)


def test_layout_transposes():
    batch, m, n, k = 2, 5, 7, 9
    c = torch.zeros(batch, n, m)
    at, bt = torch.zeros(batch, m, k), torch.zeros(batch, n, k)
    a, b = torch.zeros(batch, k, m), torch.zeros(batch, k, n)
    assert ops.ragged_batched_layout(at, b, c, trans_a=True) == (
        batch, m, n, k, k, n, m, m * k, k * n, n * m)
    assert ops.ragged_batched_layout(a, bt, c, trans_b=True) == (
        batch, m, n, k, m, k, m, k * m, n * k, n * m)
    assert ops.ragged_batched_layout(at, bt, c, True, True) == (
        batch, m, n, k, k, k, m, m * k, n * k, n * m)
    # a transposed operand's rows run along k: a row stride below K is short
    short = at.as_strided(at.shape, (m * k, k - 1, 1))
    with pytest.raises(ValueError, match="rows of a overlap"):
        ops.ragged_batched_layout(short, b, c, trans_a=True)


def test_layout_one_row_uses_width():
    # K == 1: a and b have one row, whose stride says nothing
    a = torch.zeros(2, 4, 20)[:, 1:2, 3:8]
    b = torch.zeros(2, 1, 6)
    c = torch.zeros(2, 6, 5)
    assert ops.ragged_batched_layout(a, b, c)[:7] == (2, 5, 6, 1, 5, 6, 5)


def test_layout_interleaved_heads():
    t_, h, d = 11, 3, 5
    c = torch.zeros(t_, h, d).permute(1, 0, 2)  # (B=H, N=T, M=D)
    a, b = torch.zeros(h, 4, d), torch.zeros(h, 4, t_)
    got = ops.ragged_batched_layout(a, b, c)
    assert got[:4] == (h, d, t_, 4)
    assert got[6] == h * d and got[9] == d
    # heads that leave part of the row unused are still interleaved
    wide = torch.zeros(t_, h * d + 4)
    c2 = wide.as_strided((h, t_, d), (d + 2, h * d + 4, 1))
    got = ops.ragged_batched_layout(a, b, c2)
    assert got[6] == h * d + 4 and got[9] == d + 2


def test_layout_rejects_overlapping_c():
    batch, m, n, k = 3, 5, 7, 4
    a, b, _ = tensors(batch, m, n, k)
    flat = torch.zeros(batch * n * m + 64)
    # disjoint needs a stride of (n-1)*ldc + m = n*m here; one short of it
    # is also far beyond the interleaved form ((batch-1)*stride + m <= ldc)
    c = flat.as_strided((batch, n, m), (n * m - 1, m, 1))
    with pytest.raises(ValueError, match="c entries overlap"):
        ops.ragged_batched_layout(a, b, c)
    ops.ragged_batched_layout(a, b, flat.as_strided((batch, n, m),
                                                    (n * m, m, 1)))
    # interleaved needs a stride >= m; one short of it
    ldc = batch * m
    flat = torch.zeros(n * ldc + 64)
    c = flat.as_strided((batch, n, m), (m - 1, ldc, 1))
    with pytest.raises(ValueError, match="c entries overlap"):
        ops.ragged_batched_layout(a, b, c)
    # and the last head must end inside the row: ldc one short
    c = flat.as_strided((batch, n, m), (m, ldc - 1, 1))
    with pytest.raises(ValueError, match="c entries overlap"):
        ops.ragged_batched_layout(a, b, c)
    ops.ragged_batched_layout(a, b, flat.as_strided((batch, n, m),
                                                    (m, ldc, 1)))


def test_layout_rejects():
    a, b, c = tensors(3, 6, 8, 4)
    with pytest.raises(ValueError, match="c is broadcast over the batch"):
        ops.ragged_batched_layout(a, b, c[0].unsqueeze(0).expand(3, -1, -1))
    with pytest.raises(ValueError, match="batch mismatch: a has 2"):
        ops.ragged_batched_layout(a[:2], b, c)
    with pytest.raises(ValueError, match="batch mismatch: b has 2"):
        ops.ragged_batched_layout(a, b[:2], c)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.ragged_batched_layout(a[:, :, ::2], b, c[:, :, :3])
    with pytest.raises(ValueError, match="must be float32"):
        ops.ragged_batched_layout(a.double(), b, c)
    with pytest.raises(ValueError, match="empty batch or matrix"):
        ops.ragged_batched_layout(a[:, :0], b[:, :0], c)
    with pytest.raises(ValueError, match="empty batch or matrix"):
        ops.ragged_batched_layout(a[:0], b[:0], c[:0])
    with pytest.raises(ValueError, match="disagree"):
        ops.ragged_batched_layout(a, b, c[:, :, :5])
    with pytest.raises(ValueError, match=r"c must be \(B, N, M\)"):
        ops.ragged_batched_layout(a, b, c[0])
    with pytest.raises(ValueError, match="rows of b overlap or are broadcast"):
        ops.ragged_batched_layout(a, b[:, :1].expand(-1, 4, -1), c)
    big = ops.MAX_BATCH + 1
    one = torch.zeros(1, 1)
    with pytest.raises(ValueError, match="outside 1..65535"):
        ops.ragged_batched_layout(one, one, torch.zeros(big, 1, 1))
    assert ops.ragged_batched_layout(
        one, one, torch.zeros(big - 1, 1, 1))[0] == ops.MAX_BATCH


def test_choose_tier_never_none():
    for batch in (1, 3, 64):
        for m in ODD:
            for n in ODD:
                for k in (1, 333, 4097):
                    assert ops.choose_tier_ragged_batched(
                        m, n, k, batch) in ops.TIERS


def test_choose_tier_batch_one_is_the_ragged_choice():
    for m in ODD + [64, 256, 1024, 4096]:
        for n in ODD + [64, 128, 1024, 4096]:
            for k in (1, 64, 333, 4096):
                assert (ops.choose_tier_ragged_batched(m, n, k, 1) ==
                        ops.choose_tier(m, n, k, ragged=True))


def test_choose_tier_agrees_where_a_tier_fits():
    sizes = [16, 32, 64, 96, 128, 256, 1024, 2048, 4096, 4160]
    seen = 0
    for batch in (1, 3, 64):
        for m in sizes:
            for n in sizes:
                for k in (64, 96, 1024):
                    tiled = ops.choose_tier(m, n, k, batch)
                    if tiled is not None:
                        seen += 1
                        assert ops.choose_tier_ragged_batched(
                            m, n, k, batch) == tiled
    assert seen > 100


def test_choose_tier_uses_ceil_tile_counts_times_batch():
    # 1000 x 1000: 4 x 8 = 32 huge tiles; x 12 = 384 reaches the threshold
    assert ops.choose_tier_ragged_batched(1000, 1000, 80, 12) == "huge"
    assert ops.choose_tier_ragged_batched(1000, 1000, 80, 11) != "huge"
    # skinny context product below the huge threshold: n >= 4m -> wide
    assert ops.choose_tier_ragged_batched(80, 1000, 1000, 32) == "wide"
    with pytest.raises(ValueError, match=">= 1"):
        ops.choose_tier_ragged_batched(5, 5, 5, 0)
    # choose_tier itself keeps refusing a ragged batch
    with pytest.raises(ValueError):
        ops.choose_tier(5, 5, 5, 2, ragged=True)


def test_thresholds_note():
    note = ops.RAGGED_BATCHED_THRESHOLDS_NOTE
    assert "inherited, not fitted" in note and "not measured" in note


def test_ft_bmm_argument_checks():
    x, y = torch.zeros(3, 4, 5), torch.zeros(3, 5, 6)
    with pytest.raises(ValueError, match="x must be float32"):
        ops.ft_bmm(x.double(), y)
    with pytest.raises(ValueError, match="y must be float32"):
        ops.ft_bmm(x, y.half())
    with pytest.raises(ValueError, match="inner dimension"):
        ops.ft_bmm(x, y[:, :4])
    with pytest.raises(ValueError, match="batch dimensions"):
        ops.ft_bmm(x, y[:2])
    with pytest.raises(ValueError, match="both 2-D"):
        ops.ft_bmm(x[0], y[0])
    with pytest.raises(ValueError, match="at least 2-D"):
        ops.ft_bmm(x[0, 0], y)
    with pytest.raises(ValueError, match="empty"):
        ops.ft_bmm(x[:0], y[:0])
