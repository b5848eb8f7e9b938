"""End-to-end fused ABFT with the injector at the smallest shapes that reach
the locate/correct path: one block tile by K=256 and two tiles each way,
every tier, and the huge and large tiers through both the classic
(FT_SGEMM_STREAMK=0) and the stream-K (=1) kernel — the two callers of the
shared locate_correct."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING

ABS_TOL = 1e-2
REL_TOL = 1e-2
K = 256


def check(ref, got):
    diff = (ref - got).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


def _run(tier, tiles):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    m, n = tiles * TILING[tier]["bm"], tiles * TILING[tier]["bn"]
    a, b, c = ops.make_operands(m, n, K)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.ft_sgemm(tier, a, b, c, 1.0, 0.0, inject=True)
    torch.cuda.synchronize()
    check(ref, c)


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("tier", TIERS)
def test_ft_inject_smallest_shapes(tier, tiles):
    _run(tier, tiles)


@pytest.mark.parametrize("streamk", ["0", "1"])
@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("tier", ["huge", "large"])
def test_ft_inject_classic_and_streamk(tier, tiles, streamk):
    os.environ["FT_SGEMM_STREAMK"] = streamk
    try:
        _run(tier, tiles)
    finally:
        os.environ.pop("FT_SGEMM_STREAMK", None)
