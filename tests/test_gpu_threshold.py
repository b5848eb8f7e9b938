"""The tau / inj_mag boundary of the fused kernels, end to end.

tau and inj_mag are runtime parameters; the rest of the suite runs them at
(9500, 1e4) and (100, 200) only.  Here the classic kernels run with faults
under tau (left alone, not reported, and found in C exactly where the
injector's rotation puts them), faults under tau that add up across verify
windows (the wave trips, locates nothing, touches nothing, and says so),
faults just over tau and of negative sign (all corrected), and
verify_windows of 1, 7 and far more than there are K panels.

What the device must do comes from ops.predict_injection_model and
ops.predict_injected_events on the CPU; what it did is read from C and from
the FaultReport.  C is held to the derived bound of
ft_sgemm_amd/utils/errbound.py; an injected magnitude that is meant to stay
in C enters the bound as `extra` (the accumulation carries it), a corrected
site gets the project's |alpha| * 1e-2 per fault.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TIERS, TILING, threads
from ft_sgemm_amd.utils import errbound as eb

K = 256
TAU = 9500.0
FAULT_TOL = 1e-2  # per corrected fault, tests/test_gpu_fault_report.py


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    a, b, _ = ops.make_operands(m, n, k)
    g = torch.Generator(device="cpu").manual_seed(1234)
    c0 = torch.randn((n, m), generator=g).to(a.device)
    return a, b, c0


def _shape(tier, k=K):
    return 2 * TILING[tier]["bm"], TILING[tier]["bn"], k


def _launch(monkeypatch, tier, shape, alpha, beta, tau, inj_mag,
            verify_windows=20):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    monkeypatch.setenv("FT_SGEMM_STREAMK", "0")
    a, b, c0 = _case(*shape)
    c = c0.clone()
    rep = ops.FaultReport()
    ops.ft_sgemm(tier, a, b, c, alpha, beta, inject=True, tau=tau,
                 inj_mag=inj_mag, verify_windows=verify_windows, report=rep)
    return c, rep


def _counts(r):
    return (r.tripped, r.corrected, r.uncorrected, r.unlocated, r.dropped,
            r.n_events)


def _check_left_in_c(c, shape, alpha, beta, inj_mag, model, what):
    """C == clean + alpha * inj_mag * mult: every injected fault is still
    there, at the injector's site and nowhere else."""
    a, b, c0 = _case(*shape)
    mult = model.mult.t().contiguous().double().to(c.device)  # (N, M)
    assert torch.equal(model.residue, inj_mag * model.mult.double())
    ref = eb.ref64(a, b, c0, alpha, beta) + alpha * inj_mag * mult
    e = eb.bound(a, b, c0, alpha, beta, shape[2], extra=abs(inj_mag) * mult)
    eb.assert_within(c, ref, e, what)


def _key(e):
    return (e.i, e.j, e.k_begin, e.k_end, e.status)


def _check_all_corrected(c, rep, tier, shape, alpha, beta, inj_mag, vw, what,
                         magnitudes=True):
    m, n, k = shape
    want = ops.predict_injected_events(tier, m, n, k, verify_windows=vw)
    t = TILING[tier]
    assert len(want) // ((m // t["bm"]) * (n // t["bn"])) <= threads(tier)
    sites = [(e.i, e.j) for e in want]
    assert len(set(sites)) == len(sites)
    r = rep.read()
    assert [_key(e) for e in r.events] == [_key(e) for e in want]
    assert _counts(r) == (len(want), len(want), 0, 0, 0, len(want))
    worst = max(abs(e.magnitude - inj_mag) for e in r.events)
    print(f"[magnitude] {what}: max |rc - inj_mag| = {worst:.3e}")
    for e in r.events:
        assert e.magnitude * inj_mag > 0, e  # carries the fault's sign
    if magnitudes:
        assert worst <= FAULT_TOL
    rep.raise_if_uncorrected()
    a, b, c0 = _case(*shape)
    v = torch.zeros((n, m), dtype=torch.float64)
    for i, j in sites:
        v[j, i] = 1.0
    v = v.to(c.device)
    ref = eb.ref64(a, b, c0, alpha, beta)
    left = ((c.double() - ref).abs()[v > 0] / abs(alpha)).max().item()
    print(f"[victims] {what}: worst residue / |alpha| = {left:.3e}")
    e = eb.bound(a, b, c0, alpha, beta, k) + abs(alpha) * FAULT_TOL * v
    eb.assert_within(c, ref, e, what)


# ---- (a) under tau, nothing trips ----

@pytest.mark.parametrize("alpha", [1.0, -2.0])
@pytest.mark.parametrize("tier", TIERS)
def test_sub_threshold_faults_are_left_alone(monkeypatch, tier, alpha):
    """The injector's sites, read from C itself (not from the fault log the
    locate writes): 200 per fault, no wave total near 9500."""
    shape = _shape(tier)
    model = ops.predict_injection_model(tier, *shape, TAU, 200.0)
    assert max(model.wave_totals.values()) < TAU
    assert model.tripped == 0 and int(model.mult.sum()) > 0
    c, rep = _launch(monkeypatch, tier, shape, alpha, 0.0, TAU, 200.0)
    r = rep.read()
    assert _counts(r) == (0, 0, 0, 0, 0, 0) and r.events == []
    rep.raise_if_uncorrected()
    _check_left_in_c(c, shape, alpha, 0.0, 200.0, model,
                     f"sub-threshold {tier} alpha={alpha}")


# ---- (b) under tau each, over tau together ----

@pytest.mark.parametrize("alpha", [1.0, -2.0])
@pytest.mark.parametrize("tier", TIERS)
def test_sub_threshold_faults_that_add_up(monkeypatch, tier, alpha):
    """4000 per fault: a wave's third fault takes its total over 9500 (huge:
    wave 0 takes windows 0, 4, 8, 12 and trips from window 8 on), but no
    column total does.  The verify trips, locates nothing, must leave the
    accumulators alone and must count itself as unlocated."""
    shape = _shape(tier)
    model = ops.predict_injection_model(tier, *shape, TAU, 4000.0)
    assert max(model.col_totals.values()) <= TAU
    assert (model.corrected, model.uncorrected, model.n_faults) == (0, 0, 0)
    assert model.unlocated == model.tripped
    c, rep = _launch(monkeypatch, tier, shape, alpha, 0.0, TAU, 4000.0)
    r = rep.read()
    assert _counts(r) == (model.tripped, 0, 0, model.tripped, 0, 0)
    assert r.events == []
    if model.tripped:
        with pytest.raises(RuntimeError, match="unlocated"):
            rep.raise_if_uncorrected()
    else:
        rep.raise_if_uncorrected()
    _check_left_in_c(c, shape, alpha, 0.0, 4000.0, model,
                     f"adding-up {tier} alpha={alpha}")


# ---- (c) just over tau, and a negative fault ----

@pytest.mark.parametrize("tau,inj_mag", [(9500.0, 1.05 * 9500.0),
                                         (100.0, 1.05 * 100.0),
                                         (9500.0, -1e4)])
@pytest.mark.parametrize("tier", TIERS)
def test_faults_just_over_tau_are_corrected(monkeypatch, tier, tau, inj_mag):
    shape = _shape(tier)
    model = ops.predict_injection_model(tier, *shape, tau, inj_mag)
    alpha, beta = -2.0, 1.0
    c, rep = _launch(monkeypatch, tier, shape, alpha, beta, tau, inj_mag)
    assert rep.read().corrected == model.n_faults == model.corrected
    _check_all_corrected(c, rep, tier, shape, alpha, beta, inj_mag, 20,
                         f"over-tau {tier} tau={tau} inj={inj_mag}")


# ---- (d) verify_windows ----

VW_CASES = [("huge", 256, 1), ("huge", 256, 7), ("huge", 256, 1000),
            ("huge", 208, 1), ("huge", 208, 7), ("huge", 208, 1000),
            ("small", 256, 1), ("small", 256, 7), ("small", 256, 1000)]


@pytest.mark.parametrize("tier,k,vw", VW_CASES)
def test_verify_windows(monkeypatch, tier, k, vw):
    """One window at the very end, a stride that leaves a short last window,
    more windows asked for than there are K panels; K = 208 is an odd panel
    count on the huge tier.  The magnitude of a fault that sat in the
    accumulator for a long window drifts with the roundoff at its size, so
    only its sign is asserted here; C must still come out clean."""
    shape = _shape(tier, k)
    alpha, beta = -2.0, 1.0
    c, rep = _launch(monkeypatch, tier, shape, alpha, beta, TAU, 1e4,
                     verify_windows=vw)
    _check_all_corrected(c, rep, tier, shape, alpha, beta, 1e4, vw,
                         f"verify_windows {tier} K={k} vw={vw}",
                         magnitudes=False)
