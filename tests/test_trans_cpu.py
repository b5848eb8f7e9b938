"""CPU tests of the transposed-operand rules of the ragged SGEMM
(ops.ragged_layout with trans_a / trans_b) and of ft_linear's argument
checks.  Nothing here needs the extension."""

import pytest
import torch

from ft_sgemm_amd import ops

M, N, K = 5, 7, 3
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def shapes(ta, tb, m=M, n=N, k=K):
    return ((m, k) if ta else (k, m)), ((n, k) if tb else (k, n)), (n, m)


def packed(ta, tb, m=M, n=N, k=K):
    return tuple(torch.zeros(s) for s in shapes(ta, tb, m, n, k))




@pytest.mark.parametrize("ta,tb", FLAGS)
def test_layout_packed(ta, tb):
    a, b, c = packed(ta, tb)
    assert ops.ragged_layout(a, b, c, trans_a=ta, trans_b=tb) == (
        M, N, K, K if ta else M, K if tb else N, M)


def test_layout_defaults_are_untransposed():
    a, b, c = packed(False, False)
    assert ops.ragged_layout(a, b, c) == ops.ragged_layout(
        a, b, c, trans_a=False, trans_b=False) == (M, N, K, M, N, M)


@pytest.mark.parametrize("ta,tb", FLAGS)
def test_layout_views(ta, tb):
    """x[r0:r1, c0:c1] of wider parents: the row stride is the leading
    dimension whichever way the operand lies."""
    sa, sb, sc = shapes(ta, tb)
    a = torch.zeros(sa[0] + 4, 20)[2:2 + sa[0], 3:3 + sa[1]]
    b = torch.zeros(sb[0] + 4, 30)[1:1 + sb[0], 5:5 + sb[1]]
    c = torch.zeros(sc[0] + 4, 25)[3:3 + sc[0], 1:1 + sc[1]]
    assert ops.ragged_layout(a, b, c, trans_a=ta, trans_b=tb) == (
        M, N, K, 20, 30, 25)


@pytest.mark.parametrize("ta,tb", FLAGS)
def test_layout_one_row(ta, tb):
    """A one-row tensor's leading dimension is its width, whatever stride
    torch reports for the row."""
    # a transposed operand has one row when its M (or N) is 1, an
    # untransposed one when K is 1: once with a one-row a, once with b
    for m, n, k in ((1, N, K) if ta else (M, N, 1),
                    (M, 1, K) if tb else (M, N, 1)):
        sa, sb, sc = shapes(ta, tb, m, n, k)
        a = torch.zeros(9, 40)[1:1 + sa[0], 2:2 + sa[1]]
        b = torch.zeros(9, 40)[1:1 + sb[0], 2:2 + sb[1]]
        c = torch.zeros(sc)
        assert a.shape[0] == 1 or b.shape[0] == 1
        got = ops.ragged_layout(a, b, c, trans_a=ta, trans_b=tb)
        assert got == (m, n, k, sa[1] if sa[0] == 1 else 40,
                       sb[1] if sb[0] == 1 else 40, m)


@pytest.mark.parametrize("ta,tb", FLAGS[1:])
def test_layout_refusals(ta, tb):
    a, b, c = packed(ta, tb)
    sa, sb, _ = shapes(ta, tb)
    kw = dict(trans_a=ta, trans_b=tb)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.ragged_layout(torch.zeros(sa[0], 2 * sa[1])[:, ::2], b, c, **kw)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.ragged_layout(a, torch.zeros(sb[1], sb[0]).t(), c, **kw)
    with pytest.raises(ValueError, match="overlap"):
        ops.ragged_layout(torch.zeros(sa[1]).expand(sa), b, c, **kw)
    with pytest.raises(ValueError, match="overlap"):
        ops.ragged_layout(
            a, torch.zeros(64).as_strided(sb, (sb[1] - 1, 1)), c, **kw)
    with pytest.raises(ValueError, match="float32"):
        ops.ragged_layout(a.double(), b, c, **kw)
    with pytest.raises(ValueError, match="float32"):
        ops.ragged_layout(a, b.half(), c, **kw)


@pytest.mark.parametrize("ta,tb", FLAGS[1:])
def test_layout_k_disagrees(ta, tb):
    a, _, c = packed(ta, tb)
    _, sb, _ = shapes(ta, tb, k=K + 1)
    with pytest.raises(ValueError, match="disagree"):
        ops.ragged_layout(a, torch.zeros(sb), c, trans_a=ta, trans_b=tb)
    # the untransposed reading of a transposed operand does not fit either
    with pytest.raises(ValueError, match="disagree"):
        ops.ragged_layout(*packed(ta, tb))


def test_layout_square_needs_the_flag():
    """With M == N == K every reading has consistent shapes: the flags, not
    the shapes, say how an operand lies."""
    a, b, c = (torch.zeros(4, 4) for _ in range(3))
    for ta, tb in FLAGS:
        assert ops.ragged_layout(a, b, c, trans_a=ta, trans_b=tb) == (
            4, 4, 4, 4, 4, 4)


def test_ft_linear_rejects_before_the_extension(monkeypatch):
    def boom():
        raise AssertionError("the extension was touched")
    monkeypatch.setattr(ops, "_require_ext", boom)
    x, w = torch.zeros(4, 6), torch.zeros(3, 6)
    with pytest.raises(ValueError, match="float32"):
        ops.ft_linear(x.double(), w)
    with pytest.raises(ValueError, match="float32"):
        ops.ft_linear(x, w.half())
    with pytest.raises(ValueError, match="float32"):
        ops.ft_linear(x, w, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="in_features"):
        ops.ft_linear(torch.zeros(4, 5), w)
    with pytest.raises(ValueError, match="in_features"):
        ops.ft_linear(torch.zeros(2, 4, 7), w)
    with pytest.raises(ValueError, match="bias"):
        ops.ft_linear(x, w, torch.zeros(4))


def test_ft_linear_is_exported():
    assert issubclass(ops.FTLinear, torch.nn.Linear)
    lin = ops.FTLinear(6, 3, tier="small")
    assert tuple(lin.weight.shape) == (3, 6) and lin.bias is not None
    assert lin.weight.dtype == torch.float32
