"""alpha, beta and beta == 0 on every path that writes C.

alpha is consumed in three places that share no code — the classic epilogue
(csrc/ft_kernels.hpp), the stream-K direct epilogue and sk_fixup_kernel
(csrc/ft_streamk.hpp) — plus the rocBLAS paths and the distributed panel
loop.  Every path runs the same six (alpha, beta) pairs on a non-zero C0 and
is held, element by element, to the derived fp32 bound E of
ft_sgemm_amd/utils/errbound.py against an fp64 product: a dropped, doubled
or misplaced alpha or beta is orders of magnitude outside it.

Injected runs must reproduce the FAULT-FREE result.  An element the injector
can hit is allowed |alpha| * 1e-2 more per corrected fault (the project's
bound on a correction, check_magnitudes in tests/test_gpu_fault_report.py;
the correction happens before the epilogue, hence |alpha|); every other
element keeps the clean bound.

beta == 0 must overwrite C without reading it: each path also runs at
(0.5, 0) on a C pre-filled with NaN, and with +inf.

Measured on an MI355X: the worst diff / E without injection is 0.012
(classic huge), 0.003 on the stream-K paths, 0.007 for rocBLAS, 0.037 on the
K = 32 fallback and below 0.001 for the baseline chain at K = 3072; the
worst error left on a corrected element is 5.2e-4 * |alpha| (8.8e-4 where
two panels each correct the same site), a twentieth of the allowance.  Both
rocBLAS paths already survived a NaN- or Inf-filled C at beta == 0.
"""

import functools
from typing import Callable, NamedTuple, Optional

import pytest
import torch

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING, threads
from ft_sgemm_amd.parallel.distributed import block_row_sgemm
from ft_sgemm_amd.utils import errbound as eb

gpu = pytest.mark.gpu

PAIRS = [(0.5, 0.0), (-2.0, 0.0), (-2.0, 1.0), (0.5, -1.5), (0.0, -1.5),
         (1.0, 0.0)]
FAULT_TOL = 1e-2  # per corrected fault, tests/test_gpu_fault_report.py
ENV = ("FT_SGEMM_STREAMK", "FT_SGEMM_SK_G", "FT_SGEMM_SK_DEBUG",
       "FT_SGEMM_BASELINE_MODE", "FT_SGEMM_VERIFY_EVERY")


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """Operands and a fixed non-zero C0, made once per shape and never
    modified (every run works on a copy of C0)."""
    a, b, _ = ops.make_operands(m, n, k)
    g = torch.Generator(device="cpu").manual_seed(1234)
    c0 = torch.randn((n, m), generator=g).to(a.device)
    return a, b, c0


# ---- victim-site sets V (CPU), in C's (N, M) storage ----

def classic_sites(tier, m, n, k, verify_windows=20):
    """(i, j) of every fault the classic injector places; no site repeats
    as long as a block has no more windows than threads."""
    ev = ops.predict_injected_events(tier, m, n, k, verify_windows)
    sites = [(e.i, e.j) for e in ev]
    t = TILING[tier]
    nwin = len(ev) // ((m // t["bm"]) * (n // t["bn"]))
    assert nwin <= threads(tier)
    assert len(set(sites)) == len(sites), "an injector site repeats"
    return sites


def classic_v(tier, m, n, k, verify_windows=20):
    v = torch.zeros((n, m), dtype=torch.float64)
    for i, j in classic_sites(tier, m, n, k, verify_windows):
        v[j, i] = 1.0
    return v


def streamk_v(tier, m, n):
    """Every element a stream-K injection can land on: acc[0][0][0] of any
    lane of any wave, in every tile (tests/test_gpu_fault_report.py,
    test_streamk_events).  Each (tile, 64-k window) injects once, at thread
    (w * 67 + tile * 13) % THREADS: distinct for the windows of one tile as
    long as there are no more of them than threads."""
    t = TILING[tier]
    bm, bn, wm, wn = t["bm"], t["bn"], t["wm"], t["wn"]
    mm = 32
    v = torch.zeros((n, m), dtype=torch.float64)
    for wi in range(bm // wm):
        for wj in range(bn // wn):
            for sub in range(64 // mm):
                v[wj * wn:wj * wn + mm, wi * wm + 4 * sub].fill_(1.0)
    tile = v[:bn, :bm].clone()
    return tile.repeat(n // bn, m // bm)


# ---- the paths ----

class Path(NamedTuple):
    name: str
    shape: tuple
    env: dict
    run: Callable                 # run(a, b, c, alpha, beta), in place on c
    v: Optional[Callable] = None  # () -> faults per element, or None
    engaged: bool = False         # the stream-K kernel must have run


def _plain(tier):
    return lambda a, b, c, al, be: ops.sgemm(tier, a, b, c, al, be)


def _fused(tier, inject):
    return lambda a, b, c, al, be: ops.ft_sgemm(tier, a, b, c, al, be,
                                                inject=inject)


def _baseline(a, b, c, al, be):
    _, (res_row, res_col) = ops.baseline_ft(a, b, c, al, be, panel_k=1024)
    print(f"[verdict] alpha={al} beta={be}: {res_row:.3e} {res_col:.3e}")
    assert res_row < 1.0 and res_col < 1.0, (res_row, res_col)


def _block_row(a, b, c, al, be):
    block_row_sgemm(a, b, c, panel_k=256, gemm_fn=_fused("huge", True),
                    alpha=al, beta=be)


def _paths():
    out = []
    for tier in TIERS:
        t = TILING[tier]
        shape = (2 * t["bm"], 3 * t["bn"], 192)
        env = {"FT_SGEMM_STREAMK": "0"}
        out.append(Path(f"classic-{tier}-plain", shape, env, _plain(tier)))
        out.append(Path(f"classic-{tier}-fused", shape, env,
                        _fused(tier, False)))
        out.append(Path(f"classic-{tier}-inject", shape, env,
                        _fused(tier, True),
                        functools.partial(classic_v, tier, *shape)))
    sk = {"FT_SGEMM_STREAMK": "1", "FT_SGEMM_SK_G": "7",
          "FT_SGEMM_SK_DEBUG": "1"}
    for tier in ("huge", "large"):
        out.append(Path(f"streamk-{tier}-plain", (512, 384, 640), sk,
                        _plain(tier), engaged=True))
        out.append(Path(f"streamk-{tier}-inject", (512, 384, 640), sk,
                        _fused(tier, True),
                        functools.partial(streamk_v, tier, 512, 384),
                        engaged=True))
    out.append(Path("rocblas", (512, 256, 384), {}, ops.rocblas_sgemm))
    out.append(Path("baseline-default", (512, 384, 3072), {}, _baseline))
    out.append(Path("baseline-chain", (512, 384, 3072),
                    {"FT_SGEMM_BASELINE_MODE": "chain"}, _baseline))
    classic = {"FT_SGEMM_STREAMK": "0"}
    out.append(Path("auto-plain-fallback", (100, 64, 32), classic,
                    ops.sgemm_auto))
    out.append(Path("auto-ft-fallback", (100, 64, 32), classic,
                    ops.ft_sgemm_auto))
    auto_tier = ops.choose_tier(512, 512, 512)
    assert auto_tier is not None and ops.choose_tier(100, 64, 32) is None
    out.append(Path("auto-plain-tier", (512, 512, 512), classic,
                    ops.sgemm_auto))
    out.append(Path("auto-ft-tier", (512, 512, 512), classic,
                    ops.ft_sgemm_auto,
                    functools.partial(classic_v, auto_tier, 512, 512, 512)))
    # two panels, two launches: a site can take one fault per panel
    out.append(Path("block-row-huge-inject", (512, 512, 512), classic,
                    _block_row,
                    lambda: 2.0 * classic_v("huge", 512, 512, 256)))
    return out


PATHS = _paths()
_ids = [p.name for p in PATHS]


def _run_and_check(monkeypatch, capfd, path, alpha, beta, fill=None):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, val in path.env.items():
        monkeypatch.setenv(name, val)
    m, n, k = path.shape
    a, b, c0 = _case(m, n, k)
    c = c0.clone() if fill is None else torch.full_like(c0, fill)
    capfd.readouterr()
    path.run(a, b, c, alpha, beta)
    torch.cuda.synchronize()
    if path.engaged:
        assert "ENGAGED" in capfd.readouterr().err, "stream-K did not run"
    src = c0 if fill is None else None
    ref = eb.ref64(a, b, src, alpha, beta)
    e = eb.bound(a, b, src, alpha, beta, k)
    what = f"{path.name} alpha={alpha} beta={beta} fill={fill}"
    if path.v is not None:
        v = path.v().to(c.device)
        assert v.shape == c.shape
        on = v > 0
        if alpha != 0:
            left = ((c.double() - ref).abs()[on] / abs(alpha)).max().item()
            print(f"[victims] {what}: worst residue / |alpha| = {left:.3e}")
        e = e + abs(alpha) * FAULT_TOL * v
    eb.assert_within(c, ref, e, what)


@pytest.mark.parametrize("tier", TIERS)
def test_classic_victim_sites_do_not_repeat(tier):
    """CPU: the injected allowance is per site, so no site may take two
    faults; holds while a block has no more windows than threads."""
    t = TILING[tier]
    for shape in [(2 * t["bm"], 3 * t["bn"], 192), (512, 512, 512),
                  (512, 512, 256)]:
        v = classic_v(tier, *shape)
        assert v.max() == 1.0
        assert int(v.sum()) == len(classic_sites(tier, *shape))


@pytest.mark.parametrize("tier", ["huge", "large"])
def test_streamk_victim_sites(tier):
    """CPU: the site set is acc[0][0][0] of every lane (one element per
    thread per tile), and ten windows of one tile pick ten distinct
    threads."""
    t = TILING[tier]
    v = streamk_v(tier, 512, 384)
    tiles = (512 // t["bm"]) * (384 // t["bn"])
    assert int(v.sum()) == tiles * threads(tier)
    for tile in range(tiles):
        tids = {(w * 67 + tile * 13) % threads(tier) for w in range(640 // 64)}
        assert len(tids) == 640 // 64


@gpu
@pytest.mark.parametrize("alpha,beta", PAIRS)
@pytest.mark.parametrize("path", PATHS, ids=_ids)
def test_alpha_beta(monkeypatch, capfd, path, alpha, beta):
    _run_and_check(monkeypatch, capfd, path, alpha, beta)


@gpu
def test_streamk_multi_tile_ranges_alpha_beta(monkeypatch, capfd):
    """G = 3 on 16 tiles x 16 units: every workgroup has a head partial,
    several fully-owned tiles and a tail partial."""
    path = Path("streamk-huge-plain-G3", (1024, 512, 1024),
                {"FT_SGEMM_STREAMK": "1", "FT_SGEMM_SK_G": "3",
                 "FT_SGEMM_SK_DEBUG": "1"}, _plain("huge"), engaged=True)
    _run_and_check(monkeypatch, capfd, path, -2.0, 1.0)


@gpu
@pytest.mark.parametrize("variant", ["plain", "fused", "inject"])
@pytest.mark.parametrize("tier", ["huge", "large"])
def test_streamk_two_by_two_tiles(monkeypatch, capfd, tier, variant):
    """Forced stream-K at M = 2 BM, N = 2 BN, K = 256: 4 tiles x 4 units over
    G = 3 workgroups (6/5/5 units) gives fully-owned tiles, head partials and
    tail partials, crossing the tile indexing, both strip buffers and both
    fixup slots of the staging and epilogue code the two kernels share."""
    t = TILING[tier]
    m, n = 2 * t["bm"], 2 * t["bn"]
    run = _plain(tier) if variant == "plain" else _fused(tier,
                                                        variant == "inject")
    v = (functools.partial(streamk_v, tier, m, n) if variant == "inject"
         else None)
    path = Path(f"streamk-{tier}-{variant}-2x2", (m, n, 256),
                {"FT_SGEMM_STREAMK": "1", "FT_SGEMM_SK_G": "3",
                 "FT_SGEMM_SK_DEBUG": "1"}, run, v, engaged=True)
    _run_and_check(monkeypatch, capfd, path, -2.0, 1.0)


@gpu
@pytest.mark.parametrize("fill", [float("nan"), float("inf")],
                         ids=["nan", "inf"])
@pytest.mark.parametrize("path", PATHS, ids=_ids)
def test_beta_zero_never_reads_c(monkeypatch, capfd, path, fill):
    _run_and_check(monkeypatch, capfd, path, 0.5, 0.0, fill=fill)
