// ft_ragged.hpp — ragged twin of the classic kernel (sgemm_mfma): any
// M, N, K >= 1, any leading dimensions lda >= M, ldb >= N, ldc >= M, base
// pointers with only fp32 alignment.  Built from the shared device blocks of
// ft_kernels.hpp (tile_geom, checksum_regs, verify_window, locate_correct,
// FaultCtx, glds, stage_operand), like ft_streamk.hpp, and compiled in its
// own translation units (csrc/generated/kernel_<tier>_ragged.hip): the
// tiled kernels do not change.
//
// How a shape the tile does not divide is made to fit:
//   * the grid is ceil(M/BM) x ceil(N/BN) and the panel loop runs
//     ceil(K/BK) panels;
//   * every LDS element whose row is >= M, column >= N or k >= K is staged as
//     an exact 0.0f and no out-of-range address is read, so the padded
//     accumulators are exactly zero;
//   * the segment sums (segsum_ragged_kernel) are taken over the real rows
//     only and are zero for k in [K, sstr), so the column checksums of an edge
//     tile stay exact and verify_window / locate_correct run unchanged;
//   * the epilogue writes only i < M, j < N.
// The injector keeps its rule (acc[0][0][0] of thread (w*67) % THREADS in
// every block, once per window), so a victim can lie in the padding; it is
// detected, located, corrected and logged like any other, with its true
// padded coordinates (fault_log.h).
//
// Classic decomposition only: no stream-K, no batch.

#pragma once

#include "tier_launch.hpp"

namespace ftsgemm {

// The word out-of-range staging lanes load: global_load_lds has no
// immediate-zero form, so a lane that must not touch its operand reads this.
static __device__ const float ragged_zero_word[4] = {0.f, 0.f, 0.f, 0.f};

// Which 16-byte accesses a ragged launch may use, decided on the host from the
// base pointers and leading dimensions (workgroup-uniform kernel argument).
enum RaggedFast {
  RAGGED_FAST_A = 1,  // A 16-B aligned and lda % 4 == 0
  RAGGED_FAST_B = 2,  // B 16-B aligned and ldb % 4 == 0
  RAGGED_FAST_C = 4,  // C 16-B aligned and ldc % 4 == 0
};

// Guarded twin of stage_operand: the same ROWS x BK panel into the same LDS
// layout ([k][row], element f = k*ROWS + row), 4 B per lane.  A lane whose row
// is >= rows or whose k is >= K loads ragged_zero_word instead of the
// operand: the panel's in-range elements are the bits stage_operand would
// have staged and the rest are +0.0f.
template <int ROWS, int BK, int THREADS>
__device__ __attribute__((always_inline)) inline void stage_operand_guarded(
    float* dst, const float* __restrict__ g, int ld, int rows, int K, int row0,
    int k0, int tid, int wave) {
  static_assert((ROWS * BK) % THREADS == 0, "whole 4-B passes");
  constexpr int NP = (ROWS * BK) / THREADS;
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int f = t * THREADS + tid;
    const int k = k0 + f / ROWS, i = row0 + f % ROWS;
    const float* src =
        (i < rows && k < K) ? g + i + (size_t)k * ld : ragged_zero_word;
    glds<4>(src, dst + t * THREADS + wave * 64);
  }
}

// Ragged segment sums: segsum_column for any M and leading dimension, plus
// the zero fill the ragged kernel's last panel relies on.  Launched on sstr
// blocks.  Block k < K writes, per SEG-row band (ceil(M/SEG) of them), the
// plain and the (i % SEG)-weighted sum of column k over the band's rows that
// exist (i < M): f32x4 loads where the column is 16-B aligned and four rows
// exist, scalar loads of the rows < M otherwise — the same sums in the same
// order, so a band of SEG real rows has the bits segsum_kernel gives it.
// Block k in [K, sstr) writes zeros: the last panel and the last 64-k strip
// window read those entries, and a stale NaN there times a zero B would
// poison the checksum.
template <int SEG>
__global__ __launch_bounds__(256) void segsum_ragged_kernel(
    int M, int K, int lda, int sstr, const float* __restrict__ A,
    float* __restrict__ S) {
  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  if (k >= K) {
    const int nbands = (M + SEG - 1) / SEG;
    for (int band = tid; band < nbands; band += 256) {
      S[(size_t)band * 2 * sstr + 2 * k] = 0.f;
      S[(size_t)band * 2 * sstr + 2 * k + 1] = 0.f;
    }
    return;
  }
  const float* col = A + (size_t)k * lda;
  const bool vec = ((uintptr_t)col & 15) == 0;
  constexpr int GL = SEG / 4;  // lanes per segment group (4|8|16)
  for (int base = 0; base < M; base += 1024) {
    const int idx = base + tid * 4;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (vec && idx + 4 <= M) {
      v = *(const f32x4*)(col + idx);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (idx + u < M) v[u] = col[idx + u];
    }
    float s = (v[0] + v[1]) + (v[2] + v[3]);
    const float i0 = (float)(idx % SEG);
    float w = i0 * v[0] + (i0 + 1.f) * v[1] + (i0 + 2.f) * v[2] +
              (i0 + 3.f) * v[3];
#pragma unroll
    for (int m = 1; m < GL; m <<= 1) {
      s += __shfl_xor(s, m, 64);
      w += __shfl_xor(w, m, 64);
    }
    if (idx < M && (idx % SEG) == 0) {
      S[(size_t)(idx / SEG) * 2 * sstr + 2 * k] = s;
      S[(size_t)(idx / SEG) * 2 * sstr + 2 * k + 1] = w;
    }
  }
}

// The ragged kernel.  Work decomposition, panel body, injector, verify and
// the per-element epilogue expression are sgemm_mfma's; what differs is the
// staging (fast 16-B path on a block and panel where it is legal, guarded
// 4-B path elsewhere — both give the same LDS contents, so C does not depend
// on which ran), the strip of a wave whose whole band lies below row M
// (zeros), and the guarded epilogue.
template <int BM, int BN, int BK, int WM, int WN, int MM, bool ABFT,
          bool INJECT, int OCC = 2, bool LOG = false>
__global__ __launch_bounds__(
    (tile_geom<BM, BN, BK, WM, WN, MM, ABFT>::THREADS),
    OCC) void sgemm_mfma_ragged(int M, int N, int K, int lda, int ldb, int ldc,
                                int fast, const float* __restrict__ A,
                                const float* __restrict__ B,
                                float* __restrict__ C, float alpha, float beta,
                                int verify_iters, int inject_stride, float tau,
                                float inj_mag, const float* __restrict__ SA,
                                int sstr, FaultLog flog) {
  using G = tile_geom<BM, BN, BK, WM, WN, MM, ABFT>;
  using T = typename G::T;
  constexpr int KSTEP = G::KSTEP, THREADS = G::THREADS, FM = G::FM,
                FN = G::FN, BUF = G::BUF, STRIP_OFF = G::STRIP_OFF,
                PPS = G::PPS;

  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];

  const thread_pos t = G::thread(threadIdx.x);
  const int tid = t.tid, wave = t.wave, lane = t.lane, sub = t.sub, r = t.r,
            wm_idx = t.wm_idx, wi0 = t.wi0, wj0 = t.wj0;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int im0 = bx * BM;
  const int jn0 = by * BN;

  typename T::acc_t acc[FM][FN] = {};
  checksum_regs<FN> cs;  // running column checksums of this wave's tile
  cs.clear();

  // workgroup-uniform: may this block's A / B panels take the 16-B path
  // (whole tile in range, aligned operand); the panel's k range is checked
  // per panel
  const bool a_fast = (fast & RAGGED_FAST_A) && im0 + BM <= M;
  const bool b_fast = (fast & RAGGED_FAST_B) && jn0 + BN <= N;

  auto stage = [&](int q, int k0) __attribute__((always_inline)) {
    const bool k_full = k0 + BK <= K;
    if (a_fast && k_full)
      stage_operand<BM, BK, THREADS>(&lds[q * BUF], A, lda, im0, k0, tid,
                                     wave);
    else
      stage_operand_guarded<BM, BK, THREADS>(&lds[q * BUF], A, lda, M, K, im0,
                                             k0, tid, wave);
    if (b_fast && k_full)
      stage_operand<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B, ldb, jn0, k0,
                                     tid, wave);
    else
      stage_operand_guarded<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B, ldb,
                                             N, K, jn0, k0, tid, wave);
  };

  // This wave's WM-row band of A.  The workspace holds ceil(M/WM) bands; a
  // wave whose band starts at or below row M has only padding rows, and its
  // strip is zeros.  k needs no guard: sstr >= the last window's end and the
  // segment-sum pass zero-filled [K, sstr).
  const int segA = bx * G::WAVES_M + wm_idx;
  const bool band_real = segA * WM < M;
  auto stage_strip = [&](int pb, int k0) __attribute__((always_inline)) {
    float* dst = G::strip(lds, wave, pb);
    const float* ga = SA + (size_t)segA * 2 * sstr + 2 * k0 + lane;
    glds<4>(band_real ? ga : ragged_zero_word, dst);
    glds<4>(band_real ? ga + 64 : ragged_zero_word, dst + 64);
  };

  auto verify = [&](int it_end) __attribute__((always_inline)) {
    verify_window<G, LOG>(acc, cs, sub, tau, flog, im0, jn0, 0, it_end,
                          verify_iters);
  };

  // ---- main K loop: sgemm_mfma's, over ceil(K/BK) panels ----
  stage(0, 0);
  if constexpr (ABFT) stage_strip(0, 0);  // window 0 (panels 0..PPS-1)
  FT_PARA_SYNC();
  __syncthreads();  // drains in-flight glds

  const int niter = (K + BK - 1) / BK;
  int it = 0;
  while (it < niter) {
    if constexpr (INJECT) {
      if (tid == ((unsigned)(it / inject_stride) * 67u) % THREADS)
        acc[0][0][0] += inj_mag;
    }
    const int burst_end = (it + verify_iters < niter) ? it + verify_iters
                                                      : niter;
    for (; it < burst_end; ++it) {
      const int q = it & 1;
      if (it + 1 < niter) {
        stage(q ^ 1, (it + 1) * BK);
        if constexpr (ABFT) {
          if ((it + 1) % PPS == 0)
            stage_strip(((it + 1) / PPS) & 1, (it + 1) * BK);
        }
      }
      FT_PARA_SYNC();
      const float* As = &lds[q * BUF];
      const float* Bs = &lds[q * BUF + BM * BK];
      const float* strip =
          ABFT ? &lds[STRIP_OFF + wave * 256 + ((it / PPS) & 1) * 128 +
                      (it % PPS) * BK * 2]
               : nullptr;
      // the panel body of sgemm_mfma, written out again (ft_kernels.hpp
      // says why it is not a shared function)
      constexpr int NKK = BK / KSTEP;
      constexpr bool DEFER = ABFT && defer_encode<FM, FN>;
      f32x2 swv[DEFER ? NKK : 1];
      float bv[DEFER ? NKK : 1][FN];
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
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
      __syncthreads();
      if constexpr (DEFER) {
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) asm volatile("" : "+v"(swv[kk]));
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) cs.encode(swv[kk], bv[kk]);
      }
    }
    if constexpr (ABFT) verify(it);
  }

  // ---- epilogue: alpha/beta merge on the M x N window only ----
  // Per element the tiled epilogue's expression.  f32x4 where the four rows
  // exist and C allows 16-B accesses, scalar accesses of the rows < M
  // otherwise; beta == 0 never reads C.
  const bool c_vec = (fast & RAGGED_FAST_C) != 0;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int j = jn0 + wj0 + fn * MM + r;
      if (j >= N) continue;
      const int ib = im0 + wi0 + fm * MM;
      float* colbase = C + (size_t)j * ldc + ib;
#pragma unroll
      for (int g = 0; g < G::NREG / 4; ++g) {
        const int i = ib + 4 * sub + 8 * g;
        if (i >= M) continue;
        float* p = colbase + 4 * sub + 8 * g;
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
            out[u] = alpha * acc[fm][fn][4 * g + u] + beta * prev[u];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) out[u] = alpha * acc[fm][fn][4 * g + u];
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

// Ragged launch of one tier: any M, N, K >= 1 on a ceil(M/BM) x ceil(N/BN)
// grid of sgemm_mfma_ragged.  g.lda / ldb / ldc of 0 mean packed (M, N, M).
// The workspace has one row per WM-row band of A, the last band partial.
// No allocation and no sync, so the launch can be captured.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM>
hipError_t launch_tier_ragged(const GemmArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  const int M = g.M, N = g.N, K = g.K;
  const int lda = g.lda ? g.lda : M, ldb = g.ldb ? g.ldb : N,
            ldc = g.ldc ? g.ldc : M;
  const auto fast_ok = [](const void* p, int ld) {
    return ((uintptr_t)p & 15) == 0 && ld % 4 == 0;
  };
  const int fast = (fast_ok(g.A, lda) ? RAGGED_FAST_A : 0) |
                   (fast_ok(g.B, ldb) ? RAGGED_FAST_B : 0) |
                   (fast_ok(g.C, ldc) ? RAGGED_FAST_C : 0);
  const int bk_used = abft ? BKF : BK;
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN);
  dim3 block(tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS);
  const int stride = window_stride((K + bk_used - 1) / bk_used,
                                   abft ? g.verify_windows : 1);
  Checksums cs;
  if (abft) {
    cs.sstr = abft_sstr(K);
    cs.SA = g.ws;
    RoctxRange rr("abft_encode_segsum_ragged");
    hipLaunchKernelGGL((segsum_ragged_kernel<WM>), dim3(cs.sstr), dim3(256), 0,
                       g.stream, M, K, lda, cs.sstr, g.A, g.ws);
  }
  RoctxRange rr_main(abft ? (inject ? "ft_sgemm_ragged_abft_inject"
                                    : "ft_sgemm_ragged_abft")
                          : "sgemm_ragged_plain");
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn = select_variant(
      abft, inject, flog.counters != nullptr,
      &sgemm_mfma_ragged<BM, BN, BK, WM, WN, MM, false, false>,
      [](auto inj, auto lg) {
        return &sgemm_mfma_ragged<BM, BN, BKF, WM, WN, MM, true,
                                  decltype(inj)::value, 2,
                                  decltype(lg)::value>;
      });
  hipLaunchKernelGGL(kfn, grid, block, 0, g.stream, M, N, K, lda, ldb, ldc,
                     fast, g.A, g.B, g.C, g.alpha, g.beta, stride, stride,
                     g.tau, g.inj_mag, cs.SA, cs.sstr, flog);
  return hipGetLastError();
}

}  // namespace ftsgemm
