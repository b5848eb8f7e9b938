"""Argument validation shared by the three device self-test entries
(csrc/torch_ext.cpp check_selftest_descs / selftest_args): a fragment shape
no tier has, a descriptor on the CPU and an fdesc whose case count differs
from idesc's are all rejected before anything is launched, and a valid
(1, 1, 16) case afterwards still returns the documented shapes.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from ft_sgemm_amd import ops

ABS_TOL = 1e-2  # tests/test_gpu_locate_selftest.py
REL_TOL = 1e-2
AMP = 0.9 * 16
TAU, MAG = 9500.0, 10000.0
CAPACITY = 4

ENTRIES = {
    "locate": ops.locate_selftest,
    "detect": ops.detect_selftest,
    "report": lambda *a: ops.locate_selftest_report(*a, capacity=CAPACITY),
}


def test_rejected_arguments_then_a_valid_case():
    assert ops.have_extension(), "HIP extension must be built on a GPU box"
    idesc, fdesc = ops.selftest_descriptors([([(0, 0, 2, 21, MAG)], TAU)])
    idesc, fdesc = torch.from_numpy(idesc), torch.from_numpy(fdesc)
    d_idesc, d_fdesc = idesc.cuda(), fdesc.cuda()
    long_fdesc = torch.cat([d_fdesc, d_fdesc])  # (ncases + 1, 3)

    for name, entry in ENTRIES.items():
        with pytest.raises(RuntimeError):  # in range, but no tier's shape
            entry(3, 1, 32, d_idesc, d_fdesc, AMP)
        with pytest.raises(RuntimeError):
            entry(1, 1, 16, idesc, d_fdesc, AMP)
        with pytest.raises(RuntimeError):
            entry(1, 1, 16, d_idesc, long_fdesc, AMP)

    out = ops.locate_selftest(1, 1, 16, d_idesc, d_fdesc, AMP)
    det = ops.detect_selftest(1, 1, 16, d_idesc, d_fdesc, AMP)
    tiles, counters, events = ops.locate_selftest_report(
        1, 1, 16, d_idesc, d_fdesc, AMP, capacity=CAPACITY)
    torch.cuda.synchronize()
    assert out.shape == (3, 1, 4, 64) and out.dtype == torch.float32
    assert det.shape == (1, 7, 64) and det.dtype == torch.float32
    assert tiles.shape == (1, 4, 64) and tiles.dtype == torch.float32
    assert counters.shape == (1, 5) and counters.dtype == torch.int32
    assert events.shape == (1, CAPACITY, 8) and events.dtype == torch.int32

    new, clean = out[0], out[2]
    diff = (new - clean).abs()
    rel = diff / clean.abs().clamp_min(1e-30)
    print(f"max |corrected - clean| = {diff.max().item():.3e}")
    assert not ((diff > ABS_TOL) & (rel > REL_TOL)).any()
