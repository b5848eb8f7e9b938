// tier_launch.hpp — shared launcher template; each tier is compiled in its
// own translation unit (csrc/generated/kernel_<tier>.hip) so the register
// allocator sees one tier's three variants at a time (co-compiled template
// instantiations perturb each other's codegen — measured 88 vs 112 TF on
// the fused-ABFT huge tier in a monolithic TU).
#pragma once

#include <hip/hip_runtime.h>
#include <roctracer/roctx.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "ft_core.h"
#include "ft_kernels.hpp"
#include "ft_streamk.hpp"

namespace ftsgemm {

// roctx phase ranges (SURVEY.md §5 tracing row / VERDICT r01 next #9):
// every launch phase is bracketed so `rocprofv3 --marker-trace
// --kernel-trace` shows encode / GEMM / verify spans by name.  roctx is a
// no-op unless a tracer is attached.
struct RoctxRange {
  explicit RoctxRange(const char* name) { roctxRangePush(name); }
  ~RoctxRange() { roctxRangePop(); }
};

// FT_SGEMM_STREAMK: 0 = never, 1 = force (when the shape divides),
// unset/other = auto (use stream-K when the classic tile-per-workgroup
// grid would waste >15% of a dispatch round on tail quantization).
inline int streamk_env_mode() {
  // read fresh each launch (cheap vs a kernel launch) so tests can toggle
  // the mode inside one process
  const char* e = std::getenv("FT_SGEMM_STREAMK");
  return e ? std::atoi(e) : 2;
}

// The launchers below check none of the launch rules: sgemm_tier_launch runs
// gemm_args_error (dispatch.hip) first and is the only way in.

// The checksum operand of a fused kernel: SA (g.ws, layout at
// sgemm_abft_workspace_floats) and the row stride sstr it is read with; both
// zero for a plain kernel.
struct Checksums {
  const float* SA = nullptr;
  int sstr = 0;
};

// ABFT encode, when g.abft: precompute the plain + row-weighted segment
// checksums of A (per WM-row band) into g.ws: one coalesced pass over the
// operand, ~1-2% of the GEMM at N=4096 (vs -11.6% for the in-kernel
// cooperative sums pass this replaces — tools/probe_ablate.hip).
template <int WM>
void abft_encode(const GemmArgs& g, Checksums& cs) {
  if (!g.abft) return;
  cs.sstr = abft_sstr(g.K);
  cs.SA = g.ws;
  RoctxRange rr("abft_encode_segsum");
  hipLaunchKernelGGL((segsum_kernel<WM>), dim3(g.K), dim3(256), 0, g.stream,
                     g.M, g.K, cs.sstr, g.A, g.ws);
}

// The fault log a launch runs with: the caller's when one is attached (fused
// variants only), none otherwise.  Caller-owned: no allocation, no sync, so
// the launch stays legal under graph capture.
inline FaultLog attached_log(bool abft, const FaultLog* log) {
  return (abft && log && log->counters) ? *log : FaultLog{};
}

// Picks one variant of a kernel family (all share one signature): the plain
// kernel, or the fused twin with or without the injector.  With a log
// attached (`logged`) the LOG twin runs; without one, the unlogged kernel.
// fused(inj, lg) hands out the <ABFT, INJECT = inj, LOG = lg> instantiation.
template <class K, class F>
K select_variant(bool abft, bool inject, bool logged, K plain, F fused) {
  using Y = std::true_type;
  using N = std::false_type;
  if (!abft) return plain;
  if (logged) return inject ? fused(Y{}, Y{}) : fused(N{}, Y{});
  return inject ? fused(Y{}, N{}) : fused(N{}, N{});
}

inline int device_cu_count() {
  static int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                                dev);
    return n > 0 ? n : 256;
  }();
  return cus;
}

// Stream-K launch of one tier.  Returns hipErrorNotSupported when the
// classic launch is preferable (heuristic) or the shape does not divide —
// the caller then falls through to launch_tier.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM>
hipError_t launch_tier_streamk_t(const GemmArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  const int M = g.M, N = g.N, K = g.K;
  const int mode = streamk_env_mode();
  if (mode == 0) return hipErrorNotSupported;
  if (M % BM || N % BN || K % 64 || K % (abft ? BKF : BK) || M % 4 ||
      N % 4)
    return hipErrorNotSupported;
  constexpr int THREADS = tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS;

  // The occupancy query, and with it the classic/stream-K decision and the
  // grid G, always uses the unlogged kernel: attaching a log must not change
  // the decomposition (and so the summation order of C).  Nothing needs G
  // co-resident.
  const FaultLog flog = attached_log(abft, g.log);
  const auto variant = [&](bool logged) {
    return select_variant(
        abft, inject, logged,
        &sgemm_mfma_streamk<BM, BN, BK, WM, WN, MM, false, false>,
        [](auto inj, auto lg) {
          return &sgemm_mfma_streamk<BM, BN, BKF, WM, WN, MM, true,
                                     decltype(inj)::value, 2,
                                     decltype(lg)::value>;
        });
  };
  const auto kfn = variant(false);
  const auto kfn_launch = variant(flog.counters != nullptr);
  int maxblk = 0;
  const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &maxblk, (const void*)kfn, THREADS, 0);
  const bool dbg = std::getenv("FT_SGEMM_SK_DEBUG") != nullptr;
  if (oe != hipSuccess || maxblk < 1) {
    if (dbg)
      fprintf(stderr, "[sk %dx%d] occupancy query failed: err=%d maxblk=%d\n",
              BM, BN, (int)oe, maxblk);
    return hipErrorNotSupported;
  }

  const int tiles = (M / BM) * (N / BN);
  int G0 = device_cu_count() * maxblk;
  const char* ge = std::getenv("FT_SGEMM_SK_G");  // tuning override
  if (ge) G0 = std::atoi(ge);
  if (G0 < 1) return hipErrorNotSupported;
  if (mode != 1) {
    const float rounds = ceilf((float)tiles / (float)G0);
    const float waste = (rounds * G0 - tiles) / (rounds * G0);
    // measured crossover (profiles/sk_probe r2 steady-state + CLI-protocol
    // sweeps, two-kernel fixup), huge tier.  Two usage regimes matter:
    // pipelined launches (torch/bench) amortise the per-launch fixup +
    // workspace costs and SK wins from 1024 up (+31..+98%); the
    // reference's sync-per-rep CLI protocol pays them serially, where
    // plain SK only wins in the tail-waste regime (tiles >= G/2, 3072+:
    // +5..28%) and fused SK wins from 1536 up.  Shipped gate follows the
    // sync-protocol data (the conservative one; FT_SGEMM_STREAMK=1
    // forces SK for pipelined callers):
    //   engage iff waste >= 15%, outside the ~[G/3, G/2) dead band
    //   (2560: classic 40%-fill beats the combine), and for the plain
    //   kernel only in the tail regime (2*tiles >= G).
    // maxblk > 2 (fine-grained tiers, e.g. large at 10 blocks/CU):
    // dynamic dispatch self-balances the many short blocks and SK
    // measured 15-20% WORSE at every size -> classic.
    // dead band tiles in [G/4, G/2): 2560 classic wins outright and 2048
    // SK is run-to-run bimodal (34k..94k GFLOPS across sweeps) -> classic
    const bool dead_band = (4 * tiles >= G0) && (2 * tiles < G0);
    if (maxblk > 2 || waste < 0.15f || dead_band ||
        (!abft && 2 * tiles < G0)) {
      if (dbg)
        fprintf(stderr, "[sk %dx%d] M=%d N=%d: classic (waste %.3f)\n", BM,
                BN, M, N, waste);
      return hipErrorNotSupported;
    }
  }
  const int total = tiles * (K >> 6);
  const int G = total < G0 ? total : G0;
  if (dbg)
    fprintf(stderr,
            "[sk %dx%d] M=%d N=%d K=%d: ENGAGED tiles=%d maxblk=%d G=%d "
            "units/wg~%.1f\n",
            BM, BN, M, N, K, tiles, maxblk, G, (float)total / G);

  // The owner-fixup workspace is stream-ordered (concurrent GEMMs on
  // different streams must not share it); hipMallocAsync is not legal
  // inside graph capture, so captured launches take the classic path.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(g.stream, &cap);
  if (cap != hipStreamCaptureStatusNone) return hipErrorNotSupported;

  Checksums cs;
  abft_encode<WM>(g, cs);
  RoctxRange rr_main(abft ? (inject ? "ft_sgemm_streamk_abft_inject"
                                    : "ft_sgemm_streamk_abft")
                          : "sgemm_streamk_plain");
  const int upt = K >> 6;
  const int istride = window_stride(upt, g.verify_windows);

  // split-tile partial slots: 2 per workgroup (head + tail partials).
  // One-time: raise the default mempool's release threshold so the pool
  // RETAINS this allocation across stream syncs — with the default
  // threshold (0) every sync released the 100-200 MB back to the OS and
  // each launch re-mapped it, which cost more than the whole GEMM at
  // N<=2048 in sync-per-call usage (CLI sweep: 1024 huge 19.5k steady
  // -> 8.5k with per-rep remaps).
  static const bool pool_init = [] {
    int dev = 0;
    hipMemPool_t pool = nullptr;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
      uint64_t thr = ~0ull;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold,
                                   &thr);
    }
    return true;
  }();
  (void)pool_init;
  float* partials = nullptr;
  const size_t pbytes = (size_t)2 * G * BM * BN * sizeof(float);
  if (hipMallocAsync((void**)&partials, pbytes, g.stream) != hipSuccess)
    return hipErrorNotSupported;  // nothing mutated yet; classic path

  hipLaunchKernelGGL(kfn_launch, dim3(G), dim3(THREADS), 0, g.stream, M, N, K,
                     g.A, g.B, g.C, g.alpha, g.beta, istride, g.tau,
                     g.inj_mag, cs.SA, cs.sstr, partials, flog);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) {
    // combine split tiles (fully-owned tiles exit immediately)
    hipLaunchKernelGGL((sk_fixup_kernel<BM, BN, WM, WN, MM>), dim3(tiles),
                       dim3(THREADS), 0, g.stream, M, N, upt, G, g.alpha,
                       g.beta, g.C, partials);
    err = hipGetLastError();
  }
  (void)hipFreeAsync(partials, g.stream);
  return err;
}

// BKF: K-panel depth of the fused-ABFT twin (may be smaller than the
// plain BK so the +1KB/wave checksum strips don't push the block over an
// LDS-occupancy boundary — kernel_table.py bkf note).
//
// BATCHED (g.batch > 1, instantiated in the tier's _batched translation unit
// only): g.batch GEMMs on a (M/BM, N/BN, batch) grid of the kernel's BATCHED
// twin, entry b on A + b*strideA, B + b*strideB, C + b*strideC.  strideA == 0
// shares A: its segment sums are then encoded once and read by every entry;
// otherwise g.ws holds one copy of the per-matrix workspace layout per entry.
// With a log attached, g.log is the first of g.batch logs (ft_core.h).
// Always the classic decomposition: there is no batched stream-K, and
// FT_SGEMM_STREAMK is not consulted.  No allocation and no sync on either
// path, so the launch can be captured.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool BATCHED>
hipError_t launch_tier(const GemmArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  const int M = g.M, N = g.N, K = g.K;
  const int bk_used = abft ? BKF : BK;
  dim3 grid(M / BM, N / BN, BATCHED ? g.batch : 1);
  dim3 block(tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS);
  // whole bk_used panels; a plain kernel runs them all in one burst
  const int stride = window_stride(K / bk_used, abft ? g.verify_windows : 1);
  BatchStrides bs;
  Checksums cs;
  if constexpr (!BATCHED) {
    abft_encode<WM>(g, cs);
  } else {
    bs = {g.strideA, g.strideB, g.strideC, 0};
    if (abft) {
      const int nA = g.strideA == 0 ? 1 : g.batch;
      cs.sstr = abft_sstr(K);
      cs.SA = g.ws;
      // one matrix's rows of the workspace (sgemm_abft_workspace_floats)
      const long long ws_each = 2LL * (M / WM) * cs.sstr;
      bs.SA = nA == 1 ? 0 : ws_each;
      RoctxRange rr("abft_encode_segsum_batched");
      hipLaunchKernelGGL((segsum_batched_kernel<WM>), dim3(K, nA), dim3(256),
                         0, g.stream, M, K, cs.sstr, g.A, g.ws, g.strideA,
                         ws_each);
    }
  }
  RoctxRange rr_main(
      abft ? (inject ? (BATCHED ? "ft_sgemm_batched_abft_inject"
                                : "ft_sgemm_abft_inject")
                     : (BATCHED ? "ft_sgemm_batched_abft" : "ft_sgemm_abft"))
           : (BATCHED ? "sgemm_batched_plain" : "sgemm_plain"));
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn = select_variant(
      abft, inject, flog.counters != nullptr,
      &sgemm_mfma<BM, BN, BK, WM, WN, MM, false, false, 2, false, BATCHED>,
      [](auto inj, auto lg) {
        return &sgemm_mfma<BM, BN, BKF, WM, WN, MM, true, decltype(inj)::value,
                           2, decltype(lg)::value, BATCHED>;
      });
  hipLaunchKernelGGL(kfn, grid, block, 0, g.stream, M, N, K, g.A, g.B, g.C,
                     g.alpha, g.beta, stride, stride, g.tau, g.inj_mag, cs.SA,
                     cs.sstr, flog, bs);
  return hipGetLastError();
}

}  // namespace ftsgemm
