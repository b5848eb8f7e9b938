"""GPU tests that the offline checksum chain (ops.baseline_ft, kernel id 10,
the default fallback of ops.ft_sgemm_auto) DETECTS: faults are put into the
running C through the chain's fault seam and the verdicts are held against a
derived band.

The bound (utils/errbound.py baseline_verdict_bounds has the count in full).
A row residual r_i is the difference of two fp32 quantities that are equal
in exact arithmetic, the observed row sum of C and the maintained checksum
beta * C0 e + alpha * sum_p Ap (Bp^T e).  Either is reached by at most

    ops = K + max(M, N) + 2 * npanels + 16

roundings of at most 2**-23 each, on magnitudes that sum to at most
S_i = |alpha| * sum_j P_ij + |beta| * sum_j |C0_ij| with P = |B| |A|^T, so

    |r_i| <= b_i = 2 * ops * 2**-23 * S_i,

and b_j for the columns with the sums over i.  The verdicts are the fp32
dot products res_row = sum r_i^2 and res_col = sum r_j^2, so with
d = (len + 1) * 2**-23 for that dot product's own rounding

    clean:      res_row <= (1 + d) * sum_i b_i^2
    one fault delta at (i0, j0):
        (1 - d) * (|delta| - b_d)^2 <= res_row
                 <= (1 + d) * ((|delta| + b_d)^2 + sum_i b_i^2)
        b_d = b_i0 + 2 * ops * 2**-23 * |delta|

and likewise for res_col with j0.  Two terms are added to the plain
b_i0 band: d, because the verdict is itself an fp32 sum of len terms, and
the |delta| part of b_d, because the fault is carried through the observed
side's additions like any other magnitude (at delta = 10000 and M = 1030 that
alone can be ~1, against b_i0 ~ 0.05).  Nothing is tuned to what the device
returns.  The tests rest on sum b^2 <= 200^2 / 100 at every shape, which
case() asserts; tests/test_baseline_detect_cpu.py checks the same on the
CPU and holds an fp32 emulation of the chain against the bound.

Fault magnitudes are the project's: 200.0 (tau100_mag200 of
tests/test_gpu_threshold.py) and ERROR_INJECT = 10000.0.
"""

import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import ERR_BOUND, ERROR_INJECT
from ft_sgemm_amd.utils import errbound as eb

ALPHA, BETA = 1.5, -0.5
MAG_SMALL, MAG_BIG = 200.0, ERROR_INJECT
CONDITION = MAG_SMALL ** 2 / 100  # sum b^2 must stay under this
MODES = ("default", "chain")

# (M, N, K), one panel each: the f32x4 reductions with a second row band of
# 4 rows and a ragged third column slice; the scalar reductions with a
# second band; the fallback's own test shapes; smaller than a vector; 1x1x1
SHAPES = [(1028, 132, 8), (1030, 65, 8), (100, 100, 100), (257, 129, 65),
          (3, 5, 7), (1, 1, 1)]
# five panels, the last 8 deep
CADENCE_SHAPE, CADENCE_PANEL_K, CADENCE_SITE = (64, 48, 72), 16, (21, 13)
# three panels of 40, 40, 20
NONFINITE_SHAPE, NONFINITE_PANEL_K = (100, 100, 100), 40
NONFINITE_SITE = (37, 61)


def sites(m, n):
    """Fault sites (i, j) of an M x N result: the corners, the last row of
    the f32x4 body (which M < 4 does not have), and the first row of band 2
    and first column of slice 2 where they exist; duplicates removed."""
    out = []
    for s in [(0, 0), (m - 1, n - 1), (m - 1, 0), (0, n - 1),
              ((m & ~3) - 1, n // 2), (min(m - 1, 1024), min(n - 1, 64))]:
        if s[0] >= 0 and s not in out:
            out.append(s)
    return out


def operands(m, n, k, device):
    """Seeded (a, b, c0) as tests/test_gpu_ragged.py makes them."""
    g = torch.Generator(device="cpu").manual_seed(7 * m + 3 * n + k)
    a = (torch.rand((k, m), generator=g) * 1.8 - 0.9).to(device)
    b = (torch.rand((k, n), generator=g) * 1.8 - 0.9).to(device)
    c0 = torch.randn((n, m), generator=g).to(device)
    return a, b, c0


def bounds(a, b, c0, panel_k):
    """The derived bounds of one case, from CPU tensors; asserts the
    condition the fault tests rest on."""
    k, m = a.shape
    n = b.shape[1]
    b_row, b_col = eb.baseline_verdict_bounds(a, b, c0, ALPHA, BETA, panel_k)
    out = types.SimpleNamespace(
        shape=(m, n, k), panel_k=panel_k, b_row=b_row, b_col=b_col,
        ops=eb.baseline_verdict_ops(m, n, k, panel_k),
        lim_row=eb.baseline_verdict_clean_limit(b_row),
        lim_col=eb.baseline_verdict_clean_limit(b_col))
    assert out.lim_row <= CONDITION and out.lim_col <= CONDITION, (
        f"{(m, n, k)}: sum b^2 = {out.lim_row:.4g} / {out.lim_col:.4g} is "
        f"over {CONDITION}: shrink the shape")
    return out


_cases = {}


def case(shape, panel_k):
    """One shape's operands on the GPU, fp64 reference, elementwise bound
    and verdict bounds: made once, never written."""
    if (shape, panel_k) not in _cases:
        a, b, c0 = operands(*shape, "cpu")
        cs = bounds(a, b, c0, panel_k)
        cs.a, cs.b, cs.c0 = a.cuda(), b.cuda(), c0.cuda()
        cs.ref = eb.ref64(cs.a, cs.b, cs.c0, ALPHA, BETA)
        cs.e = eb.bound(cs.a, cs.b, cs.c0, ALPHA, BETA, shape[2])
        _cases[(shape, panel_k)] = cs
    return _cases[(shape, panel_k)]


def set_env(monkeypatch, mode, every=None):
    if mode == "chain":
        monkeypatch.setenv("FT_SGEMM_BASELINE_MODE", "chain")
    else:
        monkeypatch.delenv("FT_SGEMM_BASELINE_MODE", raising=False)
    if every is None:
        monkeypatch.delenv("FT_SGEMM_VERIFY_EVERY", raising=False)
    else:
        monkeypatch.setenv("FT_SGEMM_VERIFY_EVERY", every)


def run(cs, fault=None):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    c = cs.c0.clone()
    _, pair, panels = ops.baseline_ft(cs.a, cs.b, c, ALPHA, BETA,
                                      panel_k=cs.panel_k, fault=fault,
                                      per_panel=True)
    return c, pair, panels


def assert_clean(cs, pair, what):
    rr, rc = pair
    print(f"[baseline-detect] {what} clean: res_row {rr:.4e} (limit "
          f"{cs.lim_row:.4e}), res_col {rc:.4e} (limit {cs.lim_col:.4e})")
    assert 0.0 <= rr <= cs.lim_row, f"{what}: res_row {rr} > {cs.lim_row}"
    assert 0.0 <= rc <= cs.lim_col, f"{what}: res_col {rc} > {cs.lim_col}"


def assert_faulted(cs, site, delta, pair, what):
    i, j = site
    rr, rc = pair
    lo_r, hi_r = eb.baseline_verdict_fault_band(cs.b_row, i, delta, cs.ops)
    lo_c, hi_c = eb.baseline_verdict_fault_band(cs.b_col, j, delta, cs.ops)
    print(f"[baseline-detect] {what} delta {delta} at {site}: res_row "
          f"{rr:.9g} in [{lo_r:.9g}, {hi_r:.9g}], res_col {rc:.9g} in "
          f"[{lo_c:.9g}, {hi_c:.9g}]")
    assert lo_r <= rr <= hi_r, f"{what}: res_row {rr} not in [{lo_r}, {hi_r}]"
    assert lo_c <= rc <= hi_c, f"{what}: res_col {rc} not in [{lo_c}, {hi_c}]"


def assert_result(cs, c, site=None, delta=0.0, what=""):
    """C is the product within the elementwise bound, and the fault sits on
    the one element the seam was told (c is (N, M): element (i, j) is
    c[j, i])."""
    ref, e = cs.ref, cs.e
    if site is not None:
        i, j = site
        ref, e = ref.clone(), e.clone()
        ref[j, i] += delta
        e[j, i] += 2 * eb.EPS * (abs(float(ref[j, i])) + abs(delta))
    eb.assert_within(c, ref, e, what)


SITE_CASES = [(s, st) for s in SHAPES for st in sites(s[0], s[1])]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("mode", MODES)
def test_clean_verdict_within_derived_bound(mode, shape, monkeypatch):
    set_env(monkeypatch, mode)
    cs = case(shape, shape[2])
    c, pair, panels = run(cs)
    assert [p for p, _, _ in panels] == [0]
    assert_result(cs, c, what=f"{mode} {shape}")
    assert_clean(cs, pair, f"{mode} {shape}")


@pytest.mark.parametrize("shape,site", SITE_CASES, ids=str)
@pytest.mark.parametrize("mode", MODES)
def test_every_element_is_seen(mode, shape, site, monkeypatch):
    """A reduction that skips a tail, a band or a slice misses the fault's
    200^2 in one verdict; the band is a fraction of a percent wide."""
    set_env(monkeypatch, mode)
    cs = case(shape, shape[2])
    c, pair, _ = run(cs, fault=(0, site[0], site[1], MAG_SMALL, False))
    assert_result(cs, c, site, MAG_SMALL, f"{mode} {shape} {site}")
    assert_faulted(cs, site, MAG_SMALL, pair, f"{mode} {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("mode", MODES)
def test_error_inject_magnitude_is_seen(mode, shape, monkeypatch):
    set_env(monkeypatch, mode)
    cs = case(shape, shape[2])
    site = (shape[0] - 1, shape[1] // 2)
    c, pair, _ = run(cs, fault=(0, site[0], site[1], MAG_BIG, False))
    assert_result(cs, c, site, MAG_BIG, f"{mode} {shape} {site}")
    assert_faulted(cs, site, MAG_BIG, pair, f"{mode} {shape}")
    # what ft_sgemm_auto raises on
    assert min(pair) > ERR_BOUND * ERR_BOUND


@pytest.mark.parametrize("p", range(5))
@pytest.mark.parametrize("every", [None, "1", "2", "3"])
@pytest.mark.parametrize("mode", MODES)
def test_cadence_and_worst_panel(mode, every, p, monkeypatch):
    """Which panels get a verdict, that a fault in panel p shows at the
    first verified panel >= p and at every later one, and that the returned
    pair is the worst of the list."""
    set_env(monkeypatch, mode, every)
    cs = case(CADENCE_SHAPE, CADENCE_PANEL_K)
    j = 2 if every is None else int(every)
    _, pair, panels = run(
        cs, fault=(p, CADENCE_SITE[0], CADENCE_SITE[1], MAG_BIG, False))
    assert [q for q, _, _ in panels] == [
        q for q in range(5) if (q + 1) % j == 0 or q == 4]
    for q, rr, rc in panels:
        what = f"{mode} every={every} fault in {p}, verdict of {q}"
        if q < p:
            assert_clean(cs, (rr, rc), what)
        else:
            assert_faulted(cs, CADENCE_SITE, MAG_BIG, (rr, rc), what)
    assert pair == (max(rr for _, rr, _ in panels),
                    max(rc for _, _, rc in panels))


NONFINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": -float("inf")}


@pytest.mark.parametrize("panel", [0, 2])
@pytest.mark.parametrize("kind", list(NONFINITE))
@pytest.mark.parametrize("mode", MODES)
def test_nonfinite_fault_is_not_a_clean_verdict(mode, kind, panel,
                                                monkeypatch):
    """A NaN or Inf left in one element of C makes that row's and that
    column's sum non-finite, so both verdicts must come back non-finite:
    never 0.0 (what `NaN > 0` made of it), and never the clean verdict of an
    earlier panel.  Default cadence: panels 1 and 2 are verified."""
    set_env(monkeypatch, mode)
    cs = case(NONFINITE_SHAPE, NONFINITE_PANEL_K)
    i, j = NONFINITE_SITE
    _, (rr, rc), panels = run(cs, fault=(panel, i, j, NONFINITE[kind], True))
    print(f"[baseline-detect] {mode} {kind} in panel {panel}: "
          f"({rr}, {rc}), per panel {panels}")
    assert [q for q, _, _ in panels] == [1, 2]
    assert rr != 0.0 and rc != 0.0
    assert not (rr <= cs.lim_row) and not (rc <= cs.lim_col)
    assert not math.isfinite(rr) and not math.isfinite(rc)
    for q, vr, vc in panels:
        if q < panel:
            assert_clean(cs, (vr, vc), f"{mode} {kind} verdict of {q}")
        else:
            assert not math.isfinite(vr) and not math.isfinite(vc)


AUTO_FAULTS = {kind: (value, True) for kind, value in NONFINITE.items()}
AUTO_FAULTS["1e4"] = (MAG_BIG, False)


def patch_fault(monkeypatch, fault, seen):
    """ops.baseline_ft with the fault added, recording what it returned."""
    real = ops.baseline_ft

    def faulted(*args, **kw):
        out = real(*args, fault=fault, **kw)
        seen.append(out[1])
        return out

    monkeypatch.setattr(ops, "baseline_ft", faulted)


@pytest.mark.parametrize("kind", list(AUTO_FAULTS))
@pytest.mark.parametrize("mode", MODES)
def test_auto_raises_on_a_fault(mode, kind, monkeypatch):
    set_env(monkeypatch, mode)
    shape = (100, 100, 100)
    assert ops.choose_tier(*shape) is None
    cs = case(shape, shape[2])
    value, overwrite = AUTO_FAULTS[kind]
    seen = []
    patch_fault(monkeypatch, (0, 37, 61, value, overwrite), seen)
    with pytest.raises(RuntimeError, match="offline ABFT verdict"):
        ops.ft_sgemm_auto(cs.a, cs.b, cs.c0.clone(), ALPHA, BETA)
    assert len(seen) == 1


@pytest.mark.parametrize("mode", MODES)
def test_auto_small_fault_shows_but_does_not_raise(mode, monkeypatch):
    """200.0 is under the documented 9500^2 verdict threshold: no raise, but
    the verdict carries it."""
    set_env(monkeypatch, mode)
    shape, site = (100, 100, 100), (37, 61)
    cs = case(shape, shape[2])
    seen = []
    patch_fault(monkeypatch, (0, site[0], site[1], MAG_SMALL, False), seen)
    c = ops.ft_sgemm_auto(cs.a, cs.b, cs.c0.clone(), ALPHA, BETA)
    assert_result(cs, c, site, MAG_SMALL, f"auto {mode} {shape}")
    assert len(seen) == 1
    assert_faulted(cs, site, MAG_SMALL, seen[0], f"auto {mode} {shape}")


@pytest.mark.parametrize("mode", MODES)
def test_auto_clean_does_not_raise(mode, monkeypatch):
    set_env(monkeypatch, mode)
    shape = (100, 100, 100)
    cs = case(shape, shape[2])
    seen = []
    patch_fault(monkeypatch, None, seen)
    c = ops.ft_sgemm_auto(cs.a, cs.b, cs.c0.clone(), ALPHA, BETA)
    assert_result(cs, c, what=f"auto {mode} {shape}")
    assert_clean(cs, seen[0], f"auto {mode} {shape}")


@pytest.mark.parametrize("mode", MODES)
def test_unused_seam_leaves_c_bit_identical(mode, monkeypatch):
    """fault=None is the call from before the keyword existed, and both are
    the plain rocBLAS GEMM panel by panel."""
    set_env(monkeypatch, mode)
    shape, pk = (257, 129, 65), 32
    cs = case(shape, pk)
    c_old = cs.c0.clone()
    out = ops.baseline_ft(cs.a, cs.b, c_old, ALPHA, BETA, pk)
    assert len(out) == 2 and out[0] is c_old and len(out[1]) == 2
    c_new, _, _ = run(cs, fault=None)
    c_ref = cs.c0.clone()
    for k0 in range(0, shape[2], pk):
        ops.rocblas_sgemm(cs.a[k0:k0 + pk], cs.b[k0:k0 + pk], c_ref, ALPHA,
                          BETA if k0 == 0 else 1.0)
    torch.cuda.synchronize()
    assert torch.equal(c_old, c_ref)
    assert torch.equal(c_new, c_ref)


@pytest.mark.parametrize("fault", [(3, 0, 0), (-1, 0, 0), (0, 257, 0),
                                   (0, -1, 0), (0, 0, 129), (0, 0, -1)],
                         ids=str)
def test_out_of_range_fault_raises_and_launches_nothing(fault, monkeypatch):
    set_env(monkeypatch, "default")
    shape, pk = (257, 129, 65), 32  # three panels
    cs = case(shape, pk)
    c = cs.c0.clone()
    with pytest.raises(RuntimeError, match="baseline_ft: fault"):
        ops.baseline_ft(cs.a, cs.b, c, ALPHA, BETA, panel_k=pk,
                        fault=fault + (MAG_SMALL, False))
    torch.cuda.synchronize()
    assert torch.equal(c, cs.c0)
    c, pair, _ = run(cs)
    assert_result(cs, c, what=f"after refused {fault}")
    assert_clean(cs, pair, f"after refused {fault}")
