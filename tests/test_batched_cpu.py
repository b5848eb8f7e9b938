"""CPU tests of the strided-batched SGEMM's host side: the layout helper,
BatchedFaultReport, choose_tier's batch argument, the generated batched
translation units and the batched path of block_row_sgemm (gloo)."""

import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ft_sgemm_amd import ops
from ft_sgemm_amd.kernel_table import TILING
from ft_sgemm_amd.ops import fault_report as fr
from ft_sgemm_amd.parallel.distributed import (block_row_sgemm, local_shard,
                                               torch_batched_gemm_fn,
                                               torch_gemm_fn)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, N, K = 3, 8, 12, 16


def _abc(batch=B):
    return (torch.zeros(batch, K, M), torch.zeros(batch, K, N),
            torch.zeros(batch, N, M))


def _padded(batch, rows, cols, gap):
    """(batch, rows, cols) view of a flat buffer, `gap` floats between
    entries."""
    step = rows * cols + gap
    flat = torch.zeros(batch * step)
    return flat.as_strided((batch, rows, cols), (step, cols, 1))


# ---- layout helper -------------------------------------------------------

def test_layout_contiguous():
    a, b, c = _abc()
    assert ops.batched_layout(a, b, c) == (B, M, N, K, K * M, K * N, N * M)


def test_layout_padded_strides():
    a, b, c = _padded(B, K, M, 8), _padded(B, K, N, 4), _padded(B, N, M, 12)
    assert ops.batched_layout(a, b, c) == (
        B, M, N, K, K * M + 8, K * N + 4, N * M + 12)


def test_layout_expanded_and_2d_operands_are_stride_zero():
    a, b, c = _abc()
    a1 = a[0].expand(B, K, M)
    assert ops.batched_layout(a1, b, c) == (B, M, N, K, 0, K * N, N * M)
    assert ops.batched_layout(a[0], b, c) == (B, M, N, K, 0, K * N, N * M)
    b1 = b[0].expand(B, K, N)
    assert ops.batched_layout(a, b1, c) == (B, M, N, K, K * M, 0, N * M)
    assert ops.batched_layout(a[0], b[0], c) == (B, M, N, K, 0, 0, N * M)


def test_layout_single_entry_ignores_strides():
    a, b, c = _abc(1)
    assert ops.batched_layout(a, b, c) == (1, M, N, K, 0, 0, N * M)


def _bad_layouts():
    """(id, message pattern, a, b, c)"""
    a, b, c = _abc()
    yield ("a inner dims transposed", "inner dimensions of a",
           a.transpose(1, 2).contiguous().transpose(1, 2), b, c)
    yield ("c inner dims sliced", "inner dimensions of c", a, b,
           torch.zeros(B, N, 2 * M)[:, :, :M])
    yield ("a stride not a multiple of 4", "multiples of 4",
           _padded(B, K, M, 2), b, c)
    yield ("c stride not a multiple of 4", "multiples of 4", a, b,
           _padded(B, N, M, 6))
    yield ("a batch mismatch", "batch mismatch", torch.zeros(B + 1, K, M), b,
           c)
    yield "b batch mismatch", "batch mismatch", a, torch.zeros(2, K, N), c
    yield "c broadcast", "overlap", a, b, c[0].expand(B, N, M)
    yield ("c overlapping", "overlap", a, b,
           torch.zeros(4 * N * M).as_strided((B, N, M), (N * M - 4, M, 1)))
    yield "c shape wrong", "disagree", a, b, torch.zeros(B, M, N)
    yield "c 2-D", "c must be", a, b, torch.zeros(N, M)
    yield "k mismatch", "disagree", a, torch.zeros(B, K + 4, N), c
    yield ("misaligned base", "16-byte",
           torch.zeros(B * K * M + 4)[1:1 + B * K * M].view(B, K, M), b, c)
    yield ("batch too large", "outside 1..65535", torch.zeros(K, 4),
           torch.zeros(K, 4), torch.zeros(65536, 4, 4))


@pytest.mark.parametrize("case", list(_bad_layouts()), ids=lambda t: t[0])
def test_layout_rejects(case):
    _, pattern, a, b, c = case
    with pytest.raises(ValueError, match=pattern):
        ops.batched_layout(a, b, c)


def test_layout_accepts_largest_batch():
    a, b = torch.zeros(K, 4), torch.zeros(K, 4)
    c = torch.zeros(65535, 4, 4)
    assert ops.batched_layout(a, b, c)[0] == 65535


# ---- BatchedFaultReport --------------------------------------------------

def _fill(rep, entry, events, tripped, unlocated=0):
    """Hand-write a log as the kernels would."""
    n_corr = sum(1 for e in events if e[4] == fr.STATUS_CORRECTED)
    rep.counters[entry] = torch.tensor(
        [len(events), tripped, n_corr, len(events) - n_corr, unlocated],
        dtype=torch.int32)
    for s, e in enumerate(events[:rep.capacity]):
        rep.events[entry, s] = torch.tensor(e, dtype=torch.int32)


def _ev(i, j, status, mag=1e4):
    import struct
    bits = struct.unpack("<i", struct.pack("<f", mag))[0]
    return [i, j, 0, 64, status, bits, (i if i >= 0 else 0) // 32 * 32, 32]


def test_batched_report_shapes_and_decode():
    rep = ops.BatchedFaultReport(3, capacity=4, device="cpu")
    assert rep.counters.shape == (3, fr.N_COUNTERS)
    assert rep.events.shape == (3, 4, fr.EVENT_DWORDS)
    assert rep.counters.dtype == rep.events.dtype == torch.int32
    _fill(rep, 0, [_ev(5, 7, fr.STATUS_CORRECTED),
                   _ev(1, 2, fr.STATUS_CORRECTED)], tripped=2)
    _fill(rep, 2, [_ev(40, 3, fr.STATUS_CORRECTED, -2.5)] * 6, tripped=6)
    r = rep.read()
    assert len(r) == 3
    assert [(e.i, e.j) for e in r[0].events] == [(1, 2), (5, 7)]  # sorted
    assert (r[0].n_events, r[0].corrected, r[0].tripped, r[0].dropped) == \
        (2, 2, 2, 0)
    assert r[0].events[0].magnitude == 1e4 and r[0].events[0].corrected
    assert (r[1].n_events, r[1].tripped, r[1].events) == (0, 0, [])
    assert (r[2].n_events, r[2].dropped, len(r[2].events)) == (6, 2, 4)
    assert r[2].events[0].magnitude == -2.5
    rep.raise_if_uncorrected()  # everything was corrected


def test_batched_report_raise_names_entries():
    rep = ops.BatchedFaultReport(4, capacity=2, device="cpu")
    _fill(rep, 0, [_ev(1, 1, fr.STATUS_CORRECTED)], tripped=1)
    _fill(rep, 1, [_ev(-1, 9, fr.STATUS_UNCORRECTED)], tripped=1)
    _fill(rep, 3, [], tripped=1, unlocated=1)
    with pytest.raises(RuntimeError) as ei:
        rep.raise_if_uncorrected()
    msg = str(ei.value)
    assert "[1, 3]" in msg
    assert "entry 1: 1 uncorrected" in msg and "entry 3: 0 uncorrected" in msg
    assert "entry 0" not in msg and "entry 2" not in msg


def test_batched_report_reset_and_arguments():
    rep = ops.BatchedFaultReport(2, capacity=2, device="cpu")
    _fill(rep, 1, [_ev(-1, 9, fr.STATUS_UNCORRECTED)], tripped=1)
    rep.reset()
    assert not rep.counters.any() and not rep.events.any()
    assert all(r.n_events == 0 and not r.events for r in rep.read())
    rep.raise_if_uncorrected()
    with pytest.raises(ValueError):
        ops.BatchedFaultReport(0, device="cpu")
    with pytest.raises(ValueError):
        ops.BatchedFaultReport(2, capacity=0, device="cpu")


# ---- choose_tier ---------------------------------------------------------

def _single_launch_choice(m, n, k):
    """The single-launch rule as it stood before choose_tier took a batch,
    frozen here so that the default cannot drift."""
    def fits(tier):
        t = TILING[tier]
        return m % t["bm"] == 0 and n % t["bn"] == 0 and k % t["bk"] == 0

    if fits("huge") and (m // 256) * (n // 128) >= 384:
        return "huge"
    skinny = "tall" if m >= 4 * n else "wide" if n >= 4 * m else None
    if skinny and fits(skinny):
        return skinny
    if fits("large") and (m // 64) * (n // 64) >= 1024:
        return "large"
    for tier in ("medium", "large", "small"):
        if fits(tier):
            return tier
    return None


def test_choose_tier_batch1_is_todays_answer():
    sizes = [16, 32, 48, 64, 96, 128, 256, 384, 512, 1024, 1536, 2048, 3072,
             4096, 6144, 100]
    for m in sizes:
        for n in sizes:
            for k in (16, 32, 64, 100):
                want = _single_launch_choice(m, n, k)
                assert ops.choose_tier(m, n, k) == want, (m, n, k)
                assert ops.choose_tier(m, n, k, batch=1) == want, (m, n, k)


def test_choose_tier_batched_answers_divide_the_shape():
    for m, n, k, batch in [(512, 512, 512, 64), (1024, 1024, 1024, 16),
                           (2048, 2048, 2048, 4), (96, 32, 64, 8)]:
        t = TILING[ops.choose_tier(m, n, k, batch)]
        assert m % t["bm"] == 0 and n % t["bn"] == 0 and k % t["bk"] == 0
    assert ops.choose_tier(100, 100, 100, batch=8) is None
    # the measured cells (profiles/batched_bmm.txt) and their winners
    assert ops.choose_tier(512, 512, 512, 64) == "huge"
    assert ops.choose_tier(1024, 1024, 1024, 16) == "huge"
    assert ops.choose_tier(2048, 2048, 2048, 4) == "huge"
    assert ops.choose_tier(1024, 1024, 512, 8) == "large"


# ---- generator -----------------------------------------------------------

def test_every_tier_has_a_batched_tu_matching_the_table():
    gen = os.path.join(ROOT, "csrc", "generated")
    for name, t in TILING.items():
        src = open(os.path.join(gen, f"kernel_{name}_batched.hip")).read()
        m = re.search(r"hipError_t launch_tier_batched_(\w+)\(const GemmArgs& "
                      r"g\) \{\s*return launch_tier<([^>]*), true>\(g\);",
                      src)
        assert m, name
        mm = 16 if t["mfma"] == "f32_16x16x4" else 32
        want = [t["bm"], t["bn"], t["bk"], t.get("bkf", t["bk"]), t["wm"],
                t["wn"], mm]
        assert m.group(1) == name
        assert [int(x) for x in m.group(2).split(",")] == want
    tus = [f for f in os.listdir(gen) if f.endswith("_batched.hip")
           and not f.endswith("_hip.hip")]
    assert len(tus) == len(TILING)


# ---- distributed ---------------------------------------------------------

DM, DN, DK, PANEL = 128, 96, 256, 64


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(10)
        a = torch.rand((DK, DM), generator=g) * 1.8 - 0.9
        b = torch.rand((DK, DN), generator=g) * 1.8 - 0.9
        c0 = torch.rand((DN, DM), generator=g)
        mlo, mhi = local_shard(DM, rank, world)
        nlo, nhi = local_shard(DN, rank, world)
        a_loc = a[:, mlo:mhi].contiguous()
        b_loc = b[:, nlo:nhi].contiguous()
        calls = []

        def counting(*args):
            calls.append(1)
            torch_batched_gemm_fn(*args)

        out = {}
        for key, kw in (("chunk", {}), ("batched",
                                        {"batched_gemm_fn": counting})):
            c_loc = c0[:, mlo:mhi].contiguous()
            block_row_sgemm(a_loc, b_loc, c_loc, panel_k=PANEL,
                            gemm_fn=torch_gemm_fn, alpha=1.25, beta=-1.5,
                            **kw)
            out[key] = c_loc
        ref = 1.25 * (b.transpose(0, 1) @ a[:, mlo:mhi]) - 1.5 * c0[:, mlo:mhi]
        q.put((rank, len(calls),
               torch.allclose(out["batched"], out["chunk"], rtol=0,
                              atol=1e-4),
               (out["batched"] - ref).abs().max().item()))
    finally:
        dist.destroy_process_group()


def test_block_row_sgemm_batched_world2():
    """One batched_gemm_fn call per panel gives what the per-chunk loop
    gives (tests/test_distributed.py's 1e-4)."""
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get() for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, ncalls, close, err in results:
        assert ncalls == DK // PANEL, f"rank {rank}: {ncalls} batched calls"
        assert close, f"rank {rank}: batched and per-chunk paths differ"
        assert err < 1e-4, f"rank {rank} max err {err}"


def test_torch_batched_gemm_fn_beta_zero_never_reads_c():
    g = torch.Generator().manual_seed(3)
    a = torch.rand((16, 8), generator=g)
    b = torch.rand((2, 16, 4), generator=g)
    c = torch.full((2, 4, 8), float("nan"))
    torch_batched_gemm_fn(a, b, c, 0.5, 0.0)
    ref = 0.5 * torch.bmm(b.transpose(1, 2), a.expand(2, 16, 8))
    assert torch.allclose(c, ref, rtol=0, atol=1e-6)
