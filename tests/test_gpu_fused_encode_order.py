"""Fused-ABFT encode ordering (csrc/ft_kernels.hpp panel loop, and its
stream-K twin): the strip reads are parked per panel and the checksum
encode runs behind the panel barrier, so staging or ordering mistakes show
at panel / strip-window edges.  Smallest shapes that reach each edge, run
through the public ops against a torch fp64 product, with the operand
distribution and tolerances of tests/test_gpu_kernels.py.

With injection the result must still match the FAULT-FREE product: locate
and correct only work if the deferred encode hands them the right cc/cw.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TILING

ABS_TOL = 1e-2
REL_TOL = 1e-2


def check(ref, got):
    diff = (ref - got.double()).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """Operands, a fixed non-zero C0 and the fp64 product, computed once per
    shape and never modified (every test works on a clone of C0)."""
    a, b, _ = ops.make_operands(m, n, k)
    g = torch.Generator(device="cpu").manual_seed(1234)
    c0 = torch.randn((n, m), generator=g).to(a.device)
    prod = b.double().transpose(0, 1) @ a.double()
    return a, b, c0, prod


def _run(tier, m, n, k, inject, beta):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    a, b, c0, prod = _case(m, n, k)
    c = c0.clone()
    ops.ft_sgemm(tier, a, b, c, 1.0, beta, inject=inject)
    torch.cuda.synchronize()
    check(prod + beta * c0.double(), c)


# huge (BK=16, four panels per 64-k strip window): a single panel, exactly
# one window, a window plus a partial one, two windows (strip double-buffer
# parity), an odd panel count.
HUGE_K = [16, 64, 80, 128, 208]


@pytest.mark.parametrize("beta", [0.0, -1.5])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("k", HUGE_K)
@pytest.mark.parametrize("mn", [(256, 128), (512, 256)])
def test_huge_classic(monkeypatch, mn, k, inject, beta):
    monkeypatch.setenv("FT_SGEMM_STREAMK", "0")  # pin the classic loop
    _run("huge", mn[0], mn[1], k, inject, beta)


# every other tier at its minimal tile multiple (tall and wide run their
# fused bkf=8 twin); medium and small keep the in-loop encode and pin the
# packed checksum layout for a single fragment column
OTHER = [t for t in TILING if t != "huge"]


@pytest.mark.parametrize("beta", [0.0, -1.5])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("tier", OTHER)
def test_other_tiers_classic(monkeypatch, tier, k, inject, beta):
    monkeypatch.setenv("FT_SGEMM_STREAMK", "0")
    t = TILING[tier]
    _run(tier, t["bm"], t["bn"], k, inject, beta)


@pytest.mark.parametrize("beta", [0.0, -1.5])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("k", [64, 128])
def test_huge_streamk(monkeypatch, k, inject, beta):
    """The stream-K panel loop carries the same deferred encode."""
    monkeypatch.setenv("FT_SGEMM_STREAMK", "1")
    _run("huge", 512, 256, k, inject, beta)
