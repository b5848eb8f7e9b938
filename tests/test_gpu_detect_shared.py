"""The fused kernels' shared detect (csrc/ft_kernels.hpp detect_partials) and
the per-fn partial sums it hands to locate_correct's screen.

The classic and the stream-K kernel run ONE detect; its per-fn partials
p[fn] (this lane's fp32 sum over fm and reg of acc[fm][fn][reg]) replace the
screen's own second sweep of the fragment column.  ops.detect_selftest runs
that detect and the screen (screen_passes) alone on the synthetic wave tile
of tests/test_gpu_locate_selftest.py, one wave per case, and returns the tile
it saw, the residual, the partials and the screen's verdict per fn.

Per fragment shape (huge 4x2, large 1x2, tall 2x1; MM = 32), for a single
fault of 1.05 * tau and of 0.95 * tau at every (fm, fn), reg in {0, 15},
lane in {0, 31, 32, 63}:

  * the detect trips iff the fault is over tau.  The clean residual is fp32
    rounding noise: two sums of at most 128 terms below AMP = 14.4 per lane,
    each off by at most 127 * ulp(1843) / 2 = 7.8e-3, over 64 lanes < 1.0,
    and the fault's own rounding adds 128 * ulp(1e4) / 2 = 6.3e-2 in one
    lane — against a margin of 0.05 * tau = 475 either side.
  * p[fn] equals the fp64 host sum of the same lane's accumulators to
    FM * NREG * ulp(max |acc| of that tile): an fp32 sum of n = FM * NREG
    terms is off by at most (n - 1) * ulp(largest partial sum) / 2, and the
    partial sums stay below twice the tile's largest element (the fault,
    ~1e4, against at most 64 * 14.4 = 922 of clean terms), i.e. within one
    binade of it.
  * over tau, the screen passes the faulty fn and no other.

One end-to-end case per kernel family runs the injector through the shared
detect at M=256, N=128, K=640 on the huge tier (one block, 20 verify windows
in the classic kernel): C against torch fp64 at the tolerance of
tests/test_gpu_kernels.py, the fault report against
ops.predict_injection_model.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import ERR_BOUND, ERROR_INJECT

ABS_TOL = 1e-2  # tests/test_gpu_kernels.py
REL_TOL = 1e-2
AMP = 0.9 * 16  # tests/test_gpu_locate_selftest.py
TAU = 9500.0
MM, NREG = 32, 16

# wave-tile fragment shape (FM, FN) of the tiers under test
SHAPES = {"huge": (4, 2), "large": (1, 2), "tall": (2, 1)}


def _cases(fm_n, fn_n):
    sites = [(f, fm, fn, reg, lane)
             for f in (1.05, 0.95) for fm in range(fm_n)
             for fn in range(fn_n) for reg in (0, NREG - 1)
             for lane in (0, 31, 32, 63)]
    idesc, fdesc = ops.selftest_descriptors(
        [([(fm, fn, reg, lane, f * TAU)], TAU)
         for f, fm, fn, reg, lane in sites])
    return sites, idesc, fdesc


@pytest.mark.parametrize("name", list(SHAPES))
def test_shared_detect_and_partials(name):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    fm_n, fn_n = SHAPES[name]
    e_n = fm_n * fn_n * NREG
    sites, idesc, fdesc = _cases(fm_n, fn_n)
    out = ops.detect_selftest(fm_n, fn_n, MM, torch.from_numpy(idesc).cuda(),
                              torch.from_numpy(fdesc).cuda(), AMP)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (len(sites), e_n + 1 + 2 * fn_n, 64)
    tile = out[:, :e_n, :].reshape(len(sites), fm_n, fn_n, NREG, 64)
    res = out[:, e_n, :]
    p = out[:, e_n + 1:e_n + 1 + fn_n, :]
    screen = out[:, e_n + 1 + fn_n:, :]

    # the fault really is in the tile the detect saw, at its site (clean
    # value in (-AMP, AMP) plus the fault, rounded once at the fault's size)
    over = np.array([s[0] > 1.0 for s in sites])
    for i, (f, fm, fn, reg, lane) in enumerate(sites):
        assert abs(tile[i, fm, fn, reg, lane] - fdesc[i, 0]) <= (
            AMP + np.spacing(fdesc[i, 0]))
        rest = tile[i].copy()
        rest[fm, fn, reg, lane] = 0.0
        assert np.abs(rest).max() < AMP

    # (1) trips iff over tau, the same verdict in every lane
    tripped = np.abs(res) > TAU
    assert (tripped == tripped[:, :1]).all(), "residual is not wave-uniform"
    worst = np.abs(np.abs(res[:, 0]) - fdesc[:, 0]).max()
    print(f"{name}: {len(sites)} cases, max ||res| - |fault|| = {worst:.3e}")
    wrong = np.nonzero(tripped[:, 0] != over)[0]
    assert wrong.size == 0, (
        f"detect verdict wrong in cases {[sites[i] for i in wrong[:8]]}, "
        f"res {res[wrong[:8], 0]}")

    # (2) p[fn] against the fp64 sum of the same lane's accumulators
    want = tile.astype(np.float64).sum(axis=(1, 3))  # (case, fn, lane)
    tol = fm_n * NREG * np.spacing(
        np.abs(tile).max(axis=(1, 2, 3, 4)).astype(np.float32))
    err = np.abs(p.astype(np.float64) - want).max(axis=(1, 2))
    print(f"{name}: max |p - fp64 sum| = {err.max():.3e}, "
          f"bound {tol.min():.3e}")
    wrong = np.nonzero(err > tol)[0]
    assert wrong.size == 0, (
        f"p off in cases {[sites[i] for i in wrong[:8]]}: {err[wrong[:8]]} "
        f"> {tol[wrong[:8]]}")

    # (3) the screen: wave-uniform; over tau the faulty fn passes, and a
    # clean fn never does
    assert ((screen == 0.0) | (screen == 1.0)).all()
    assert (screen == screen[:, :, :1]).all(), "screen is not wave-uniform"
    for i, (f, fm, fn, reg, lane) in enumerate(sites):
        for g in range(fn_n):
            if g != fn:
                assert screen[i, g, 0] == 0.0, (sites[i], g)
            elif f > 1.0:
                assert screen[i, g, 0] == 1.0, (sites[i], g)


M_E2E, N_E2E, K_E2E = 256, 128, 640
_e2e = {}


def _e2e_operands():
    """(a, b, fp64 reference), computed once and never written."""
    if not _e2e:
        a, b, _ = ops.make_operands(M_E2E, N_E2E, K_E2E)
        _e2e["v"] = (a, b, b.double().t() @ a.double())
    return _e2e["v"]


@pytest.mark.parametrize("streamk", ["0", "1"])
def test_injector_end_to_end(monkeypatch, streamk):
    """huge, one block tile.  Classic: K/BK = 40 panels, 20 windows of 2.
    Stream-K (forced): 10 work units of 64 k on 10 workgroups, one inject +
    verify group each, so the model is evaluated at 10 windows; its victim
    rotation is the classic kernel's, so for stream-K the counts are
    compared and not the sites."""
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    monkeypatch.setenv("FT_SGEMM_STREAMK", streamk)
    a, b, ref = _e2e_operands()
    c = torch.zeros((N_E2E, M_E2E), device="cuda")
    rep = ops.FaultReport()
    ops.ft_sgemm("huge", a, b, c, 1.0, 0.0, inject=True, report=rep)
    r = rep.read()

    windows = 20 if streamk == "0" else K_E2E // 64
    model = ops.predict_injection_model("huge", M_E2E, N_E2E, K_E2E,
                                        ERR_BOUND, ERROR_INJECT,
                                        verify_windows=windows)
    assert model.tripped == model.corrected == windows
    assert (r.tripped, r.corrected, r.uncorrected, r.unlocated, r.n_events,
            r.dropped) == (model.tripped, model.corrected, model.uncorrected,
                           model.unlocated, model.n_faults, 0)
    if streamk == "0":
        want = ops.predict_injected_events("huge", M_E2E, N_E2E, K_E2E)
        assert [(e.i, e.j, e.k_begin, e.k_end, e.status) for e in r.events] \
            == [(e.i, e.j, e.k_begin, e.k_end, e.status) for e in want]
    worst = max(abs(e.magnitude - ERROR_INJECT) for e in r.events)
    print(f"stream-K={streamk}: max |rc - inj_mag| = {worst:.3e}")

    diff = (ref - c.double()).abs()
    rel = diff / ref.abs().clamp_min(1e-30)
    bad = (diff > ABS_TOL) & (rel > REL_TOL)
    print(f"stream-K={streamk}: max |C - fp64| = {diff.max().item():.3e}")
    assert not bad.any(), (
        f"{int(bad.sum())} mismatches, max abs diff {diff.max().item():.4e}")
