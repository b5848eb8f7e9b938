"""Stream-K kernel correctness (csrc/ft_streamk.hpp): the work-centric
decomposition that fixes the grid-straggler sweep sizes (VERDICT r01 next
#3).  FT_SGEMM_STREAMK=1 forces the stream-K path so these tests pin it
regardless of the auto heuristic; every case is checked against the plain
torch fp32 reference, the fused cases with the always-on 20-fault
injector (split tiles must verify+correct their PARTIAL accumulations)."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops

ABS_TOL = 1e-2
REL_TOL = 1e-2


@pytest.fixture(autouse=True)
def force_streamk():
    os.environ["FT_SGEMM_STREAMK"] = "1"
    yield
    os.environ.pop("FT_SGEMM_STREAMK", None)


def check(ref, got):
    diff = (ref - got).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")


# shapes chosen to cover: tiles < G (full split regime), a straggler grid,
# single-tile (all units in one tile), and K smaller than one 64-k unit
# per split boundary behaviour
SHAPES = [(1024, 1024, 1024), (3072, 3072, 3072), (256, 128, 2048),
          (512, 384, 640), (2048, 2048, 192)]


@pytest.mark.parametrize("tier", ["huge", "large"])
@pytest.mark.parametrize("shape", SHAPES)
def test_streamk_plain(tier, shape):
    m, n, k = shape
    if any(d % t != 0 for d, t in
           [(m, 256 if tier == "huge" else 64),
            (n, 128 if tier == "huge" else 64), (k, 64)]):
        pytest.skip("shape does not divide this tier")
    a, b, c = ops.make_operands(m, n, k)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.sgemm(tier, a, b, c, 1.0, 0.0)
    torch.cuda.synchronize()
    check(ref, c)


@pytest.mark.parametrize("tier", ["huge", "large"])
@pytest.mark.parametrize("shape", SHAPES)
def test_streamk_fused_inject(tier, shape):
    m, n, k = shape
    if any(d % t != 0 for d, t in
           [(m, 256 if tier == "huge" else 64),
            (n, 128 if tier == "huge" else 64), (k, 64)]):
        pytest.skip("shape does not divide this tier")
    a, b, c = ops.make_operands(m, n, k)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.ft_sgemm(tier, a, b, c, 1.0, 0.0, inject=True)
    torch.cuda.synchronize()
    check(ref, c)


def test_streamk_beta_prescale():
    """beta is applied exactly once per output element: by the direct
    epilogue for tiles one workgroup owns fully, by sk_fixup_kernel (after
    it has summed the raw partial slots) for split tiles."""
    m = n = k = 1024
    a, b, c = ops.make_operands(m, n, k)
    c.normal_()
    c0 = c.clone()
    ref = ops.torch_reference(a, b, c0, 1.0, -1.5)
    ops.ft_sgemm("huge", a, b, c, 1.0, -1.5, inject=True)
    torch.cuda.synchronize()
    check(ref, c)


def test_streamk_off_env():
    """FT_SGEMM_STREAMK=0 must take the classic path (same numerics)."""
    os.environ["FT_SGEMM_STREAMK"] = "0"
    m = n = k = 1024
    a, b, c = ops.make_operands(m, n, k)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.ft_sgemm("huge", a, b, c, 1.0, 0.0, inject=True)
    torch.cuda.synchronize()
    check(ref, c)


def test_streamk_k_not_multiple_of_64_falls_back():
    """K % 64 != 0 is outside the stream-K unit quantum: the wrapper must
    fall back to the classic kernel even when forced."""
    m, n, k = 512, 256, 80  # k % 16 == 0 but k % 64 != 0
    a, b, c = ops.make_operands(m, n, k)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.ft_sgemm("huge", a, b, c, 1.0, 0.0, inject=True)
    torch.cuda.synchronize()
    check(ref, c)


@pytest.mark.parametrize("g", [3, 8, 17])
def test_streamk_multi_segment_workgroups(g):
    """Workgroup ranges LONGER than one tile (q > upt): each workgroup has
    a head partial, full middle tiles, and a tail partial — the shape
    class where the retired owner-spin protocol deadlocked on partial
    dispatch (N=4608 in the r2 evidence sweep).  A tiny forced G makes
    every workgroup span multiple tiles deterministically, covering both
    fixup slots and the g0==gl early-exit."""
    os.environ["FT_SGEMM_SK_G"] = str(g)
    try:
        m, n, k = 1024, 512, 1024   # huge tier: 16 tiles x 16 units
        a, b, c = ops.make_operands(m, n, k)
        ref = ops.torch_reference(a, b, c, 1.0, -0.5)
        ops.sgemm("huge", a, b, c, 1.0, -0.5)
        torch.cuda.synchronize()
        check(ref, c)
        a, b, c = ops.make_operands(m, n, k)
        ref = ops.torch_reference(a, b, c, 1.0, 0.0)
        ops.ft_sgemm("huge", a, b, c, 1.0, 0.0, inject=True)
        torch.cuda.synchronize()
        check(ref, c)
    finally:
        os.environ.pop("FT_SGEMM_SK_G", None)


@pytest.mark.parametrize("tier", ["huge", "large"])
def test_streamk_beta_all_epilogue_paths(tier):
    """beta != 0 through every path that writes C, on both stream-K tiers.
    (512, 384, 640) divides both tiles and is 10 units per tile; G=7 gives
    every workgroup a head partial, fully-owned tiles and a tail partial
    (huge: 60 units in ranges of 9/9/9/9/8/8/8; large: 480 units in
    69/69/69/69/68/68/68), so the direct epilogue, both fixup slots and
    the fixup's g0 == gl early-out all run with C pre-filled."""
    os.environ["FT_SGEMM_SK_G"] = "7"
    try:
        m, n, k = 512, 384, 640
        a, b, c = ops.make_operands(m, n, k)
        c.normal_()
        c0 = c.clone()
        ref = ops.torch_reference(a, b, c0, 1.0, -1.5)
        ops.sgemm(tier, a, b, c, 1.0, -1.5)
        torch.cuda.synchronize()
        check(ref, c)
        c.copy_(c0)
        ops.ft_sgemm(tier, a, b, c, 1.0, -1.5, inject=True)
        torch.cuda.synchronize()
        check(ref, c)
    finally:
        os.environ.pop("FT_SGEMM_SK_G", None)


def test_streamk_high_fault_rate():
    """Dense verify windows on split tiles: istride drops to 1 (one
    inject+verify per 64-k window per tile segment)."""
    m = n = k = 2048
    a, b, c = ops.make_operands(m, n, k)
    ref = ops.torch_reference(a, b, c, 1.0, 0.0)
    ops.ft_sgemm("huge", a, b, c, 1.0, 0.0, inject=True, verify_windows=64)
    torch.cuda.synchronize()
    check(ref, c)
