// ft_ragged_streamk.hpp — stream-K for the single ragged launch: the work walk
// of sgemm_mfma_streamk (ft_streamk.hpp) with the staging and the guards of
// sgemm_mfma_ragged (ft_ragged.hpp).  Any M, N, K >= 1, any leading
// dimension, transposed operands, plain and fused-ABFT with injector and fault
// log.  Compiled in its own translation units
// (csrc/generated/kernel_<tier>_ragged_sk_{nn,tn,nt,tt}.hip): neither parent
// kernel changes.
//
// Why: the classic ragged launch runs one workgroup per output tile, so a
// product with few tiles and a deep K (a layer's grad_weight: out x in tiles,
// K = tokens) leaves most of the chip idle, and one just above a dispatch
// round pays a nearly empty tail round.  Here the work is the list of
//   total = ceil(M/BM) * ceil(N/BN) * ceil(K/64)
// units, a unit being one 64-k window of one tile (the granularity the
// checksum strips are staged at), k fastest, cut into G balanced contiguous
// ranges, one per workgroup.  The last unit of a tile is short when
// K % 64 != 0: a segment that ends in it runs
// ceil((min(K, 64*w_hi) - 64*w_lo) / BK) panels, the last of them staged
// through the guarded path, which zero-fills k >= K.
//
// Split tiles are combined as in ft_streamk.hpp, by a second kernel and in a
// fixed order (the tail partial of the tile's first workgroup, then the head
// partials of the following workgroups in workgroup order): no atomics, no
// flags, no residency assumption, and the same bits on every run.  The
// partial slots are whole BM x BN tiles, padding included, so they need no
// guards; only the epilogues know M, N and ldc.  The slots live in a
// caller-owned buffer (GemmArgs::sk_partials), so the launch allocates
// nothing and can be captured.
//
// A tile that one workgroup owns whole runs the panels of the classic ragged
// kernel in the same order and takes its epilogue: its elements of C have the
// bits of the classic ragged launch.
//
// ABFT composes as in ft_streamk.hpp: the checksums cover exactly the k range
// a segment accumulated, verify runs once per `istride` units counted from
// the segment start and at segment end, and everything is corrected before a
// partial leaves the registers.  The injector keeps the tiled stream-K rule,
// per (tile, unit group); a victim in the zero padding is a padded event, as
// in the ragged launch.

#pragma once

#include "ft_ragged.hpp"

namespace ftsgemm {

// The guarded alpha/beta epilogue of sgemm_mfma_ragged on thread t's TPT
// values v (element (fm*FN + fn)*NREG + reg) of tile (im0, jn0): only i < M,
// j < N is touched, f32x4 where four rows exist and c_vec allows 16-B
// accesses, and beta == 0 never reads C.  Used by the fixup pass; the main
// kernel writes it out on its accumulators, as both parent kernels do
// (docs/ABLATION.md §5e).
template <class G>
__device__ __attribute__((always_inline)) inline void ragged_epilogue(
    const float (&v)[G::TPT], const thread_pos& t, int im0, int jn0, int M,
    int N, int ldc, bool c_vec, float alpha, float beta,
    float* __restrict__ C) {
#pragma unroll
  for (int fm = 0; fm < G::FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < G::FN; ++fn) {
      const int j = jn0 + t.wj0 + fn * G::MM + t.r;
      if (j >= N) continue;
      const int ib = im0 + t.wi0 + fm * G::MM;
      float* colbase = C + (size_t)j * ldc + ib;
#pragma unroll
      for (int g4 = 0; g4 < G::NREG / 4; ++g4) {
        const int i = ib + 4 * t.sub + 8 * g4;
        if (i >= M) continue;
        float* p = colbase + 4 * t.sub + 8 * g4;
        const int e = (fm * G::FN + fn) * G::NREG + 4 * g4;
        const bool whole = c_vec && i + 4 <= M;
        f32x4 out;
        if (beta != 0.f) {
          f32x4 prev{0.f, 0.f, 0.f, 0.f};
          if (whole) {
            prev = *(const f32x4*)p;
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (i + u < M) prev[u] = p[u];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            out[u] = alpha * v[e + u] + beta * prev[u];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) out[u] = alpha * v[e + u];
        }
        if (whole) {
          *(f32x4*)p = out;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (i + u < M) p[u] = out[u];
        }
      }
    }
}

// sk_fixup_kernel for a ragged launch: ceil tile counts, ldc and the guarded
// epilogue; the slots and the summation order are unchanged.  One workgroup
// per tile with the main kernel's thread geometry; a tile one workgroup owns
// whole was written by the main kernel and exits at once.
template <int BM, int BN, int WM, int WN, int MM>
static __global__ __launch_bounds__(
    (tile_geom<BM, BN, 64, WM, WN, MM, false>::THREADS))
void sk_fixup_ragged_kernel(int M, int N, int ldc, int fast, int upt, int nwg,
                            float alpha, float beta, float* __restrict__ C,
                            const float* __restrict__ partials) {
  using G = tile_geom<BM, BN, 64, WM, WN, MM, false>;
  const int tile = blockIdx.x;
  const int ntm = (M + BM - 1) / BM;
  const int total = ntm * ((N + BN - 1) / BN) * upt;
  const int q = total / nwg, rem = total % nwg;
  const int g0 = sk_wg_of_unit(tile * upt, q, rem);
  const int gl = sk_wg_of_unit(tile * upt + upt - 1, q, rem);
  if (g0 == gl) return;  // fully owned -> already epilogued

  const thread_pos t = G::thread(threadIdx.x);
  // g0's tail partial (slot 2*g0+1), then every head partial in (g0, gl]
  float s[G::TPT];
  load_partial<G, false>(s, partial_slot<G>(partials, 2 * g0 + 1, t.tid));
  for (int gc = g0 + 1; gc <= gl; ++gc)
    load_partial<G, true>(s, partial_slot<G>(partials, 2 * gc, t.tid));
  ragged_epilogue<G>(s, t, (tile % ntm) * BM, (tile / ntm) * BN, M, N, ldc,
                     (fast & RAGGED_FAST_C) != 0, alpha, beta, C);
}

// The ragged stream-K kernel, on dim3(G) workgroups.  Per segment (one
// workgroup's part of one tile, units [w_lo, w_hi)) it is sgemm_mfma_ragged
// on the k range [64*w_lo, min(K, 64*w_hi)): the same staging, SPLIT rule,
// panel body and verify, restarted behind the previous segment's closing
// barrier.  What a segment leaves is the guarded epilogue when it is the
// whole tile, a raw partial in slot 2g (head, w_lo > 0) or 2g+1 (tail)
// otherwise.
template <int BM, int BN, int BK, int WM, int WN, int MM, bool ABFT,
          bool INJECT, int OCC = 2, bool LOG = false, bool TA = false,
          bool TB = false>
__global__ __launch_bounds__(
    (tile_geom<BM, BN, BK, WM, WN, MM, ABFT>::THREADS),
    OCC) void sgemm_mfma_ragged_streamk(int M, int N, int K, int lda, int ldb,
                                        int ldc, int fast,
                                        const float* __restrict__ A,
                                        const float* __restrict__ B,
                                        float* __restrict__ C, float alpha,
                                        float beta, int istride, float tau,
                                        float inj_mag,
                                        const float* __restrict__ SA, int sstr,
                                        float* __restrict__ partials,
                                        FaultLog flog) {
  using G = tile_geom<BM, BN, BK, WM, WN, MM, ABFT>;
  using T = typename G::T;
  constexpr int KSTEP = G::KSTEP, THREADS = G::THREADS, FM = G::FM,
                FN = G::FN, BUF = G::BUF, STRIP_OFF = G::STRIP_OFF,
                PPS = G::PPS;  // PPS panels = one whole 64-k work unit
  static_assert(64 % BK == 0 && BK <= 64, "stream-K unit is 64 k");

  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];

  const thread_pos t = G::thread(threadIdx.x);
  const int tid = t.tid, wave = t.wave, lane = t.lane, sub = t.sub, r = t.r,
            wm_idx = t.wm_idx, wi0 = t.wi0, wj0 = t.wj0;

  const int ntm = (M + BM - 1) / BM;
  const int upt = (K + 63) >> 6;  // units per tile, the last may be short
  const int total = ntm * ((N + BN - 1) / BN) * upt;
  // balanced contiguous unit ranges: the first (total % gridDim.x)
  // workgroups take one extra unit
  const int wg = blockIdx.x;
  const int q = total / gridDim.x, rem = total % gridDim.x;
  int u = wg * q + (wg < rem ? wg : rem);
  const int u_end = u + q + (wg < rem ? 1 : 0);

  // the segment's tile; all workgroup-uniform, set at each segment start
  int im0 = 0, jn0 = 0, segA = 0;
  bool a_fast = false, b_fast = false, band_real = false;

  using StA = stage_operand_t<BM, BK, THREADS>;
  using StB = stage_operand_t<BN, BK, THREADS>;
  typename StA::regs ra;  // a transposed operand's next panel (fast path)
  typename StB::regs rb;
  constexpr bool SPLIT = TA && TB;  // ft_ragged.hpp says why
  // A alone transposed: its registers are loaded half way through the MFMA
  // loop, not before it.  The walk's own state costs this kernel about ten
  // VGPRs over sgemm_mfma_ragged, and with ra held across the whole loop the
  // fused huge TN kernels spilled (docs/ABLATION.md section 19).  Half a
  // panel of MFMAs still covers the load; the LDS image is the same.
  constexpr bool LATE_A = TA && !TB;

  // stage / stage_mid / stage_finish of sgemm_mfma_ragged, written out again,
  // with LATE_A added
  auto load_b_t = [&](int k0) __attribute__((always_inline)) {
    if (b_fast && k0 + BK <= K) StB::load(rb, B, ldb, jn0, k0, tid);
  };
  auto store_a_t = [&](int qb, int k0) __attribute__((always_inline)) {
    if (a_fast && k0 + BK <= K) StA::store(ra, &lds[qb * BUF], tid);
  };
  auto stage = [&](int qb, int k0) __attribute__((always_inline)) {
    const bool k_full = k0 + BK <= K;
    if constexpr (TA) {
      if (a_fast && k_full) {
        if constexpr (!LATE_A) StA::load(ra, A, lda, im0, k0, tid);
      } else
        stage_operand_guarded_t<BM, BK, THREADS>(&lds[qb * BUF], A, lda, M, K,
                                                 im0, k0, tid, wave);
    } else {
      if (a_fast && k_full)
        stage_operand<BM, BK, THREADS>(&lds[qb * BUF], A, lda, im0, k0, tid,
                                       wave);
      else
        stage_operand_guarded<BM, BK, THREADS>(&lds[qb * BUF], A, lda, M, K,
                                               im0, k0, tid, wave);
    }
    if constexpr (TB) {
      if constexpr (!SPLIT) load_b_t(k0);
      if (!(b_fast && k_full))
        stage_operand_guarded_t<BN, BK, THREADS>(&lds[qb * BUF + BM * BK], B,
                                                 ldb, N, K, jn0, k0, tid,
                                                 wave);
    } else {
      if (b_fast && k_full)
        stage_operand<BN, BK, THREADS>(&lds[qb * BUF + BM * BK], B, ldb, jn0,
                                       k0, tid, wave);
      else
        stage_operand_guarded<BN, BK, THREADS>(&lds[qb * BUF + BM * BK], B,
                                               ldb, N, K, jn0, k0, tid, wave);
    }
  };
  auto stage_mid = [&](int qb, int k0) __attribute__((always_inline)) {
    if constexpr (SPLIT) {
      store_a_t(qb, k0);
      load_b_t(k0);
    }
    if constexpr (LATE_A) {
      if (a_fast && k0 + BK <= K) StA::load(ra, A, lda, im0, k0, tid);
    }
  };
  auto stage_finish = [&](int qb, int k0) __attribute__((always_inline)) {
    if constexpr (TA || TB) {
      if constexpr (TA && !SPLIT) store_a_t(qb, k0);
      if constexpr (TB) {
        if (b_fast && k0 + BK <= K)
          StB::store(rb, &lds[qb * BUF + BM * BK], tid);
      }
      FT_PARA_SYNC();
    }
  };
  // A band with no real row reads zeros.  k needs no guard: sstr covers the
  // last unit whole and the segment-sum pass zero-filled [K, sstr).
  auto stage_strip = [&](int pb, int k0) __attribute__((always_inline)) {
    float* dst = G::strip(lds, wave, pb);
    const float* ga = SA + (size_t)segA * 2 * sstr + 2 * k0 + lane;
    glds<4>(band_real ? ga : ragged_zero_word, dst);
    glds<4>(band_real ? ga + 64 : ragged_zero_word, dst + 64);
  };

  // Declared once, outside the tile loop, and re-zeroed per segment
  // (ft_streamk.hpp says why).
  typename T::acc_t acc[FM][FN];
  checksum_regs<FN> cs;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = {};
  cs.clear();

  auto verify = [&](int kbase, int p_end, int ppg)
      __attribute__((always_inline)) {
    verify_window<G, LOG>(acc, cs, sub, tau, flog, im0, jn0, kbase, p_end,
                          ppg);
  };

  const bool c_vec = (fast & RAGGED_FAST_C) != 0;

  while (u < u_end) {
    const int tile = u / upt;
    const int w_lo = u - tile * upt;
    const int seg_units = (u_end - u < upt - w_lo) ? (u_end - u)
                                                   : (upt - w_lo);
    const int w_hi = w_lo + seg_units;
    const int bx = tile % ntm, by = tile / ntm;
    im0 = bx * BM, jn0 = by * BN;
    segA = bx * G::WAVES_M + wm_idx;
    band_real = segA * WM < M;
    a_fast = (fast & RAGGED_FAST_A) && im0 + BM <= M;
    b_fast = (fast & RAGGED_FAST_B) && jn0 + BN <= N;
    const int kbase = w_lo << 6;
    const int kend = (w_hi << 6) < K ? (w_hi << 6) : K;
    const int npan = (kend - kbase + BK - 1) / BK;

    // behind the previous segment's closing barrier: both buffers are free
    stage(0, kbase);
    stage_mid(0, kbase);
    stage_finish(0, kbase);
    if constexpr (ABFT) stage_strip(w_lo & 1, kbase);
    FT_PARA_SYNC();
    __syncthreads();

    const int PPG = istride * PPS;  // panels per inject+verify group
    int p = 0;
    while (p < npan) {
      if constexpr (INJECT) {
        // deterministic rotating victim per (tile, unit group)
        if (tid == ((unsigned)((w_lo + p / PPS) * 67u + tile * 13u) %
                    THREADS))
          acc[0][0][0] += inj_mag;
      }
      const int burst_end = (p + PPG < npan) ? p + PPG : npan;
      for (; p < burst_end; ++p) {
        const int qb = p & 1;
        if (p + 1 < npan) {
          stage(qb ^ 1, kbase + (p + 1) * BK);
          if constexpr (ABFT) {
            if ((p + 1) % PPS == 0)
              stage_strip((w_lo + (p + 1) / PPS) & 1, kbase + (p + 1) * BK);
          }
        }
        FT_PARA_SYNC();
        const float* As = &lds[qb * BUF];
        const float* Bs = &lds[qb * BUF + BM * BK];
        const float* strip =
            ABFT ? &lds[STRIP_OFF + wave * 256 + ((w_lo + p / PPS) & 1) * 128 +
                        (p % PPS) * BK * 2]
                 : nullptr;
        // the panel body of sgemm_mfma, written out again (ft_kernels.hpp
        // says why it is not a shared function)
        constexpr int NKK = BK / KSTEP;
        constexpr bool DEFER = ABFT && defer_encode<FM, FN>;
        f32x2 swv[DEFER ? NKK : 1];
        float bv[DEFER ? NKK : 1][FN];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          if constexpr (SPLIT || LATE_A) {
            if (kk == NKK / 2 && p + 1 < npan)
              stage_mid(qb ^ 1, kbase + (p + 1) * BK);
          }
          const int kloc = kk * KSTEP + sub;
          float a[FM], b[FN];
#pragma unroll
          for (int fm = 0; fm < FM; ++fm)
            a[fm] = As[kloc * BM + wi0 + fm * MM + r];
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            b[fn] = Bs[kloc * BN + wj0 + fn * MM + r];
          if constexpr (DEFER) {
            swv[kk] = *(const f32x2*)(strip + 2 * kloc);
#pragma unroll
            for (int fn = 0; fn < FN; ++fn) bv[kk][fn] = b[fn];
          } else if constexpr (ABFT) {
            cs.encode(*(const f32x2*)(strip + 2 * kloc), b);
          }
          __builtin_amdgcn_iglp_opt(0);
#pragma unroll
          for (int fm = 0; fm < FM; ++fm)
#pragma unroll
            for (int fn = 0; fn < FN; ++fn)
              acc[fm][fn] = T::mma(a[fm], b[fn], acc[fm][fn]);
        }
        if (p + 1 < npan) stage_finish(qb ^ 1, kbase + (p + 1) * BK);
        __syncthreads();
        if constexpr (DEFER) {
#pragma unroll
          for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(swv[kk]));
#pragma unroll
          for (int kk = 0; kk < NKK; ++kk) cs.encode(swv[kk], bv[kk]);
        }
      }
      if constexpr (ABFT) verify(kbase, p, PPG);
    }

    // ---- tile contribution (ft_streamk.hpp has the protocol) ----
    const bool full_seg = (w_lo == 0) && (w_hi == upt);
    if (!full_seg) {
      store_partial<G>(
          partial_slot<G>(partials, 2 * wg + (w_lo == 0 ? 1 : 0), t.tid), acc);
    } else {
      // the guarded epilogue of sgemm_mfma_ragged, written out on the
      // accumulators (the fixup pass has it as ragged_epilogue)
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
          const int j = jn0 + wj0 + fn * MM + r;
          if (j >= N) continue;
          const int ib = im0 + wi0 + fm * MM;
          float* colbase = C + (size_t)j * ldc + ib;
#pragma unroll
          for (int g4 = 0; g4 < G::NREG / 4; ++g4) {
            const int i = ib + 4 * sub + 8 * g4;
            if (i >= M) continue;
            float* p4 = colbase + 4 * sub + 8 * g4;
            const bool whole = c_vec && i + 4 <= M;
            f32x4 out;
            if (beta != 0.f) {
              f32x4 prev{0.f, 0.f, 0.f, 0.f};
              if (whole) {
                prev = *(const f32x4*)p4;
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (i + e < M) prev[e] = p4[e];
              }
#pragma unroll
              for (int e = 0; e < 4; ++e)
                out[e] = alpha * acc[fm][fn][4 * g4 + e] + beta * prev[e];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                out[e] = alpha * acc[fm][fn][4 * g4 + e];
            }
            if (whole) {
              *(f32x4*)p4 = out;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (i + e < M) p4[e] = out[e];
            }
          }
        }
    }
    u += seg_units;
    if (u < u_end) {  // re-zero for the next tile segment
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = {};
      if constexpr (ABFT) cs.clear();
    }
  }
}

// The variant of the family g selects; `logged` picks the LOG twin.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM, bool TA,
          bool TB>
auto ragged_streamk_variant(const GemmArgs& g, bool logged) {
  return select_variant(
      g.abft, g.inject, logged,
      &sgemm_mfma_ragged_streamk<BM, BN, BK, WM, WN, MM, false, false, 2,
                                 false, TA, TB>,
      [](auto inj, auto lg) {
        return &sgemm_mfma_ragged_streamk<BM, BN, BKF, WM, WN, MM, true,
                                          decltype(inj)::value, 2,
                                          decltype(lg)::value, TA, TB>;
      });
}

// Workgroups per CU of the variant g selects, always the unlogged one:
// attaching a log must not change the device grid (the rule of
// launch_tier_streamk_t).  0 when the query fails.  Launches nothing.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false>
int ragged_streamk_occupancy(const GemmArgs& g) {
  constexpr int THREADS = tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS;
  int maxblk = 0;
  const auto kfn =
      ragged_streamk_variant<BM, BN, BK, BKF, WM, WN, MM, TA, TB>(g, false);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &maxblk, (const void*)kfn, THREADS, 0) != hipSuccess)
    return 0;
  return maxblk > 0 ? maxblk : 0;
}

// Ragged stream-K launch of one tier on g.sk_grid workgroups (clamped to the
// unit count): the ragged encode, the main kernel, the fixup pass.  TA / TB
// must equal g.transA / g.transB, as for launch_tier_ragged.  Checks nothing
// (gemm_args_error does).  No allocation, no sync, no environment lookup and
// no mempool call: the launch can be captured.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false>
hipError_t launch_tier_ragged_streamk(const GemmArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  const int M = g.M, N = g.N, K = g.K;
  const int lda = g.lda ? g.lda : (TA ? K : M),
            ldb = g.ldb ? g.ldb : (TB ? K : N), ldc = g.ldc ? g.ldc : M;
  const int fast = ragged_fast_bits(g, lda, ldb, ldc);
  constexpr int THREADS = tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS;
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const int upt = (K + 63) >> 6;
  const int total = tiles * upt;
  const int G = g.sk_grid < total ? g.sk_grid : total;
  const int istride = window_stride(upt, g.verify_windows);
  BatchStrides bs;
  Checksums cs;
  ragged_encode<WM, TA>(g, lda, cs, bs);
  RoctxRange rr_main(abft ? (inject ? "ft_sgemm_ragged_streamk_abft_inject"
                                    : "ft_sgemm_ragged_streamk_abft")
                          : "sgemm_ragged_streamk_plain");
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn = ragged_streamk_variant<BM, BN, BK, BKF, WM, WN, MM, TA, TB>(
      g, flog.counters != nullptr);
  hipLaunchKernelGGL(kfn, dim3(G), dim3(THREADS), 0, g.stream, M, N, K, lda,
                     ldb, ldc, fast, g.A, g.B, g.C, g.alpha, g.beta, istride,
                     g.tau, g.inj_mag, cs.SA, cs.sstr, g.sk_partials, flog);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  // combine split tiles (fully-owned tiles exit immediately)
  hipLaunchKernelGGL((sk_fixup_ragged_kernel<BM, BN, WM, WN, MM>), dim3(tiles),
                     dim3(THREADS), 0, g.stream, M, N, ldc, fast, upt, G,
                     g.alpha, g.beta, g.C, (const float*)g.sk_partials);
  return hipGetLastError();
}

}  // namespace ftsgemm
