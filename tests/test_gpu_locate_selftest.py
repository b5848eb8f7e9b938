"""Device self-test of the shared ABFT locate/correct (csrc/ft_kernels.hpp
locate_correct, driven by csrc/locate_selftest.hip).

ft_sgemm's injector only ever hits acc[0][0][0], so a fault in a second
fragment column or a lower fragment row — the fragments locate_correct is
allowed to SKIP — cannot be produced end to end.  The self-test kernel
plants faults at arbitrary (fm, fn, reg, lane) sites of a synthetic wave
tile and corrects it twice: with the shipped function and with the
sweep-everything form it replaced (locate_correct_ref).  Per tier shape:

  * every single-fault site, no fault, two faults in different columns of
    one fn, two faults in different fn, two faults in one column (the
    documented blended / fail-safe outcome), 1.01*tau and 0.99*tau faults,
    tau=100 with a 200.0 fault;
  * shipped == reference BIT FOR BIT in every case;
  * correctable cases restore the clean tile within the corrected-output
    tolerance of tests/test_gpu_kernels.py.

Why that tolerance holds at AMP = 0.9*16 (accumulator magnitudes of a
16-deep panel of uniform(-0.9, 0.9) operands): the subtracted magnitude rc
is (fp64 column sum) - (fp32 checksum).  A lane's checksum is an fp32 sum of
at most 64 terms bounded by AMP, so its rounding error is at most
64 adds * 2^-24 * 64*AMP = 3.5e-3, plus ulp(1e4)/2 = 4.9e-4 each for the
final subtraction and the fp32 cast of rc: 4.5e-3 < ABS_TOL = 1e-2.  The
row index is round(rw/rc) with rw an fp32 weighted sum whose terms stay
below 127*1e4: at most 64 adds * ulp(1.27e6)/2 = 4 of error against
|rc| >= 100, i.e. 0.04 of a row.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops

ABS_TOL = 1e-2  # tests/test_gpu_kernels.py
REL_TOL = 1e-2
AMP = 0.9 * 16
TAU, MAG = 9500.0, 10000.0

# wave-tile fragment shape (FM, FN, MM) of every tier
SHAPES = {"huge": (4, 2, 32), "tall": (2, 1, 32), "large_wide": (1, 2, 32),
          "medium": (1, 1, 32), "small": (1, 1, 16)}


def _cases(fm_n, fn_n, mm):
    """-> (idesc, fdesc, correctable mask, names of the special cases)."""
    nreg = 16 if mm == 32 else 4
    rows = []  # (faults [(fm, fn, reg, lane, mag)], tau, correctable)
    for fm in range(fm_n):
        for fn in range(fn_n):
            for reg in range(nreg):
                for lane in range(64):
                    rows.append(([(fm, fn, reg, lane, MAG)], TAU, True))
    special = {}

    def add(name, faults, tau, ok):
        special[name] = len(rows)
        rows.append((faults, tau, ok))

    add("none", [], TAU, True)
    # lanes 3 and 17 hold different columns for both MM (3 vs 17 / 3 vs 1)
    add("two_lanes_one_fn", [(0, 0, 1, 3, MAG), (fm_n - 1, 0, nreg - 1, 17,
                                                 -MAG)], TAU, True)
    if fn_n > 1:
        add("two_fn", [(0, 0, 5 % nreg, 7, MAG),
                       (fm_n - 1, fn_n - 1, 2, 40, 1.5 * MAG)], TAU, True)
    # lanes 9 and 9+MM: same column, different rows -> blended, match ref
    add("same_column", [(0, 0, 0, 9, MAG), (fm_n - 1, 0, nreg - 1, 9 + mm,
                                            MAG)], TAU, False)
    add("just_above_tau", [(fm_n - 1, fn_n - 1, 3, 21, 1.01 * TAU)], TAU,
        True)
    # below the threshold nothing may be touched: not "corrected", only ref
    add("just_below_tau", [(fm_n - 1, fn_n - 1, 3, 21, 0.99 * TAU)], TAU,
        False)
    add("tau100_mag200", [(fm_n - 1, fn_n - 1, 2, 50, 200.0)], 100.0, True)

    idesc, fdesc = ops.selftest_descriptors([r[:2] for r in rows])
    ok = np.array([r[2] for r in rows])
    return idesc, fdesc, ok, special


@pytest.mark.parametrize("name", list(SHAPES))
def test_locate_correct_matches_reference(name):
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    fm_n, fn_n, mm = SHAPES[name]
    idesc, fdesc, ok, special = _cases(fm_n, fn_n, mm)
    out = ops.locate_selftest(fm_n, fn_n, mm,
                              torch.from_numpy(idesc).cuda(),
                              torch.from_numpy(fdesc).cuda(), AMP)
    torch.cuda.synchronize()
    new, ref, clean = out[0], out[1], out[2]

    # the inputs really were faulty where a fault was planted: the clean
    # tile is in (-AMP, AMP) and non-trivial
    assert clean.abs().max().item() < AMP and clean.abs().mean().item() > 1.0

    same = (new.view(torch.int32) == ref.view(torch.int32)).flatten(1).all(1)
    bad_cases = (~same).nonzero().flatten().tolist()
    assert not bad_cases, (
        f"shipped != reference in {len(bad_cases)} cases, first "
        f"{bad_cases[:8]} (special: {special})")

    okm = torch.from_numpy(ok).cuda()
    diff = (new - clean).abs()
    rel = diff / clean.abs().clamp_min(1e-30)
    bad = ((diff > ABS_TOL) & (rel > REL_TOL)).flatten(1).any(1) & okm
    print(f"{name}: {len(ok)} cases, max |corrected - clean| over "
          f"correctable cases {diff[okm].max().item():.3e}")
    assert not bad.any(), (
        f"not restored in cases {bad.nonzero().flatten().tolist()[:8]} "
        f"(special: {special}), max diff {diff[okm].max().item():.3e}")

    # sub-threshold fault: detected by nobody, left exactly as planted
    i = special["just_below_tau"]
    assert abs((new[i] - clean[i]).abs().max().item() - 0.99 * TAU) < 1.0
