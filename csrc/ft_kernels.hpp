// ft_kernels.hpp — MI355X (gfx950/CDNA4) fault-tolerant SGEMM kernel family.
//
// Brand-new design with the capabilities of the reference CUDA kernel library
// (/root/reference/kernel/ft_sgemm/include_code_gen/*.cuh, algorithm traced
// in SURVEY.md §2.3), re-architected for CDNA4:
//
//   * f32-input MFMA outer products (v_mfma_f32_32x32x2_f32 for the
//     32x32-fragment tiers, v_mfma_f32_16x16x4_f32 for the small tier) —
//     exact fp32 numerics at the 157 TF/s f32 vector rate.
//   * LDS double-buffered A/B K-panels staged with global_load_lds
//     (async HBM->LDS DMA, 16 B per lane), one __syncthreads per K-panel.
//   * Checksum ENCODE from precomputed segment sums: a separate
//     bandwidth-bound kernel (segsum_kernel) computes, per WM-row band of
//     A, the plain and the row-index-weighted column sums in one coalesced
//     pass (~1-2% of GEMM time at N=4096); the fused kernel streams each
//     wave's 64-k strip of them into a private LDS strip with one
//     4-B-per-lane global_load_lds per panel pair.  This replaces the
//     reference's per-k-step in-loop shuffle encode
//     (ft_sgemm_huge.cuh:150-213) and the earlier in-kernel cooperative
//     panel-sums pass: ablation (tools/probe_ablate.hip) measured the
//     in-kernel sums pass + its extra barrier at -11.6% of plain GEMM
//     throughput, vs ~2% for the precompute pass.
//   * 64-lane-wavefront ABFT verify with RATIO LOCATE: each wave maintains
//     per-lane column checksums (plain cc + row-weighted cw) of its output
//     sub-tile.  A fault's column is lane-local (MFMA acc column == lane %
//     MM), its magnitude is the plain column residual rc, and its row is
//     round(rw/rc) — no cross-lane row reductions at all, unlike the
//     reference's block-wide LDS transpose-reduce + row x col intersection
//     (ft_sgemm_huge.cuh:346-485).
//   * periodic in-kernel verify -> ratio locate -> branch-free in-register
//     correction, and a deterministic rotating fault injector (template
//     flag, not hard-coded: SURVEY.md §5 asks for measurable overhead with
//     and without injection).
//
// Matrix semantics (reference parity, sgemm.cu:108): C = alpha*A*B^T + beta*C,
// A MxK / B NxK / C MxN, all column-major.  Host launchers require
// M % BM == 0, N % BN == 0, K % BK == 0 and M,N multiples of 4 (the sweep
// sizes 1024..6144 step 512 and the distributed N=32768 all satisfy this).

#pragma once

#include <hip/hip_runtime.h>

#include "fault_log.h"

// FT_PARANOID (race-check build, `make cli-paranoid`): drain ALL
// outstanding async staging (glds vmcnt + LDS lgkm) and barrier right at
// every staging site.  Per-thread arithmetic order is unchanged, so the
// output must be BIT-IDENTICAL to the normal build; any difference is a
// staging race (SURVEY.md §5 race-detection row).
#ifdef FT_PARANOID
#define FT_PARA_SYNC()                                                  \
  do {                                                                  \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");         \
    __syncthreads();                                                    \
  } while (0)
#else
#define FT_PARA_SYNC() \
  do {                 \
  } while (0)
#endif

namespace ftsgemm {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

template <int MM> struct mfma_traits;

// v_mfma_f32_32x32x2_f32: lane l holds A[i=l&31][k=l>>5], B[k=l>>5][j=l&31];
// C/D: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5), reg in [0,16).
template <> struct mfma_traits<32> {
  static constexpr int kstep = 2;
  static constexpr int nreg = 16;
  using acc_t = f32x16;
  static __device__ inline acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
};

// v_mfma_f32_16x16x4_f32: lane l holds A[i=l&15][k=l>>4], B[k=l>>4][j=l&15];
// C/D: col = lane&15, row = (lane>>4)*4 + reg, reg in [0,4).
template <> struct mfma_traits<16> {
  static constexpr int kstep = 4;
  static constexpr int nreg = 4;
  using acc_t = f32x4;
  static __device__ inline acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
};

// Completes a per-k-slice partial into a full sum across the 64/MM slices
// (masks MM..32).
template <int MM> __device__ inline float slice_sum(float v) {
#pragma unroll
  for (int m = MM; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Double-precision variant for the cold locate path (shuffles the two
// 32-bit halves).
template <int MM> __device__ inline double dslice_sum(double v) {
#pragma unroll
  for (int m = MM; m < 64; m <<= 1) {
    union { double d; int i[2]; } u{v};
    u.i[0] = __shfl_xor(u.i[0], m, 64);
    u.i[1] = __shfl_xor(u.i[1], m, 64);
    v += u.d;
  }
  return v;
}

// Accumulator register -> row within the MM x MM fragment (valid for both
// MFMA shapes used here; for MM=16, reg>>2 == 0).
__device__ constexpr int acc_row(int reg, int sub) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * sub;
}

// One lane's running column checksums of its wave tile: per fragment column
// fn the plain checksum cc (col r of frag fn, this lane's k-slices only) and
// the row-index-weighted one cw (ratio locate: fault row =
// round(residual(cw) / residual(cc))).  They live in register PAIRS laid
// out so that each encode step is a whole v_pk_fma_f32 whose broadcast
// operand is a half the instruction can select by itself (op_sel), with no
// v_mov to build it (docs/ABLATION.md §5b):
//   FN even: v[2j] = (cc[2j], cc[2j+1]), v[2j+1] = (cw[2j], cw[2j+1]) —
//            the B pair is used as loaded, the segment sum is broadcast;
//   FN odd:  v[fn] = (cc[fn], cw[fn]) — the segment-sum pair is used as
//            loaded, the B value is broadcast.
// Every component is one fused multiply-add per k-slice, in ascending k:
// the same bits as the scalar fmaf chain.
template <int FN> struct checksum_regs {
  static constexpr bool PAIRED = FN % 2 == 0;
  f32x2 v[FN];
  __device__ inline void clear() {
#pragma unroll
    for (int i = 0; i < FN; ++i) v[i] = f32x2{0.f, 0.f};
  }
  // sw = (plain, row-weighted) segment sum of this lane's k-slice
  __device__ inline void encode(f32x2 sw, const float (&b)[FN]) {
    if constexpr (PAIRED) {
#pragma unroll
      for (int j = 0; j < FN / 2; ++j) {
        const f32x2 bp{b[2 * j], b[2 * j + 1]};
        v[2 * j] = __builtin_elementwise_fma(f32x2{sw[0], sw[0]}, bp, v[2 * j]);
        v[2 * j + 1] =
            __builtin_elementwise_fma(f32x2{sw[1], sw[1]}, bp, v[2 * j + 1]);
      }
    } else {
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        v[fn] = __builtin_elementwise_fma(sw, f32x2{b[fn], b[fn]}, v[fn]);
    }
  }
  __device__ inline float cc(int fn) const {
    return PAIRED ? v[fn & ~1][fn & 1] : v[fn][0];
  }
  __device__ inline float cw(int fn) const {
    return PAIRED ? v[fn | 1][fn & 1] : v[fn][1];
  }
};

// Whether the fused panel loop parks its strip reads and runs the encode
// behind the panel barrier (see the panel loop of sgemm_mfma).  The
// single-fragment tiers (medium, small: one MFMA per k-step) keep the encode
// next to its read: deferring removes no LGKM drain from their loop, and
// costs the small tier 10 VGPRs and with them a wave of occupancy.
template <int FM, int FN> constexpr bool defer_encode = FM * FN > 1;

// What locate_correct needs to report a fault: the log and where the wave
// tile sits.  (i0, j0) is the wave tile's first global row / column,
// [k_begin, k_end) the verify window (classic) or work-unit group
// (stream-K) whose accumulation is being checked.
struct FaultCtx {
  FaultLog log;
  int i0 = 0, j0 = 0, k_begin = 0, k_end = 0;
};

// Cheap detect of one wave tile, shared by the classic and the stream-K
// kernel (and run every verify window by every wave): compares the total
// tile sum against the total checksum.  Returns the wave-uniform residual
// and hands out p[fn], this lane's fp32 sum over fm and reg of
// acc[fm][fn][reg], which locate_correct screens the fragment columns with
// instead of sweeping them again.  The order of these sums is free: res and
// p only gate branches and never reach C.  Per fn two independent chains of
// packed adds run over the accumulators' own aligned register pairs (0,1),
// (2,3), ..., so every step is a v_pk_add_f32 on registers as they lie, with
// no move to build an operand, and FN * 2 chains are in flight instead of one
// FM*FN*NREG-deep scalar chain (docs/ABLATION.md §5d).
template <int FM, int FN, int MM>
__device__ __attribute__((always_inline)) inline float detect_partials(
    const typename mfma_traits<MM>::acc_t (&acc)[FM][FN],
    const float (&cc)[FN], float (&p)[FN]) {
  constexpr int NREG = mfma_traits<MM>::nreg;
  constexpr int PPF = NREG / 2;  // register pairs per fragment
  constexpr int NP = FM * PPF;   // register pairs per fragment column
  static_assert(NP % 2 == 0, "two chains of whole register pairs");
  // The residual is formed from the pair sums, not from p: p[fn] is then
  // only read in the tripped branch, and its two halves are folded there.
  // With FN even the checksums leave as the pairs (cc[2j], cc[2j+1]) they
  // are kept in (checksum_regs), one packed subtract each; scalar adds of
  // them next to the fold of tot were packed through three v_mov_b32.
  f32x2 tot;
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    f32x2 s[2];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const typename mfma_traits<MM>::acc_t& a = acc[i / PPF][fn];
      const int reg = 2 * (i % PPF);
      const f32x2 v{a[reg], a[reg + 1]};
      s[i & 1] = i < 2 ? v : s[i & 1] + v;
    }
    const f32x2 t = s[0] + s[1];
    p[fn] = t[0] + t[1];
    tot = fn == 0 ? t : tot + t;
  }
  float res;
  if constexpr (FN % 2 == 0) {
#pragma unroll
    for (int j = 0; j < FN / 2; ++j) tot -= f32x2{cc[2 * j], cc[2 * j + 1]};
    res = tot[0] + tot[1];
  } else {
    res = tot[0];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) res -= cc[fn];
    res += tot[1];
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) res += __shfl_xor(res, m, 64);
  return res;
}

// The fp32 screen of one fragment column, from the detect's partial p and
// this lane's checksum partial cc: wave-uniform, true when some lane's column
// residual exceeds tau/2.  The exact decision in locate_correct is |rc| > tau
// on the fp64 sum; the two residuals differ by the fp32 rounding of FM*NREG
// terms (~1e-2 at the |acc| ~ 1e4 of a faulty column), orders of magnitude
// below the tau/2 margin, so the screen passes a strict superset.
template <int MM>
__device__ __attribute__((always_inline)) inline bool screen_passes(
    float p, float cc, float tau) {
  const float rc32 = slice_sum<MM>(p - cc);
  // Opaque copy of tau for the screen only.  Measured, not reasoned:
  // without it the K-panel loop of the huge no-injection kernel is
  // scheduled slightly differently and runs 0.6% slower; with it the
  // loop is nearly the unscreened kernel's (docs/ABLATION.md §5a).
  float tau_o = tau;
  asm volatile("" : "+v"(tau_o));
  return __any(fabsf(rc32) > 0.5f * tau_o) != 0;
}

// ABFT ratio locate + in-register correct of one wave tile, shared by the
// classic and the stream-K kernel (entered only after the cheap detect in
// verify_window tripped; the scheme itself is described in sgemm_mfma).
// acc[FM][FN] is the wave's accumulator tile, cc/cw this lane's plain and
// row-weighted column-checksum partials, p the per-fn partial sums the
// detect (detect_partials) just formed of the same acc, sub = lane / MM.
//
// Only the work a fault needs is done:
//   * per fn, an fp32 SCREEN of the column residual (screen_passes, on the
//     detect's p[fn]: the column is not summed a second time) decides
//     whether the fragment column is looked at at all.
//   * per fm, the correction sweep runs only for a fragment some lane
//     located its row in.
// The arithmetic on a column that IS processed is the unscreened one, in
// the same order, so outputs are bit-identical to sweeping everything.
//
// This is also the ONE place that writes the fault log (fault_log.h), for
// both callers, in the LOG instantiation only: a null-pointer test in one
// shared instantiation cost every fused kernel 2-5 VGPRs and the tall tier
// a wave of occupancy (docs/ABLATION.md §5c), so the launchers pick the LOG
// twin when a log is attached and the kernels that run without one are the
// unlogged code.  ctx is built by the caller inside its tripped branch.
// Per entry: tripped += 1; per bad column one event, counted
// as corrected when the located row is inside the wave tile and as
// uncorrected (the fail-safe) otherwise; unlocated += 1 when no column was
// bad.  After the slice sums rc and row are identical in the 64/MM lanes
// that share a column, so the lane with sub == 0 reports for all of them.
// The log only reads what the locate computed: acc is corrected exactly as
// without it.
template <int FM, int FN, int MM, bool LOG = false>
__device__ __attribute__((always_inline)) inline void locate_correct(
    typename mfma_traits<MM>::acc_t (&acc)[FM][FN], const float (&cc)[FN],
    const float (&cw)[FN], const float (&p)[FN], int sub, float tau,
    const FaultCtx& ctx = FaultCtx{}) {
  constexpr int NREG = mfma_traits<MM>::nreg;
  bool any_bad = false;
  if constexpr (LOG) {
    if (__lane_id() == 0) atomicAdd(ctx.log.counters + FLOG_TRIPPED, 1);
  }
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    // With a single fragment column (FN == 1) the tripped detect already
    // says the fault is in it: no screen (it would only add code — and on
    // the tall tier two VGPRs that cost a wave of occupancy).
    if constexpr (FN > 1) {
      if (!screen_passes<MM>(p[fn], cc[fn], tau)) continue;
    }

    // fp64 PLAIN column sum: the fault itself (|e| ~ 1e4) sits in this
    // sum, so an fp32 accumulation rounds every later term at ulp(1e4)
    // ~ 1e-3 and the CORRECTION (rc is subtracted from the output)
    // inherits ~5e-3..1e-2 of error (found by tools/soak.py at
    // |alpha| > 1).  The WEIGHTED sum stays fp32: rw only selects an
    // integer row via round(rw/rc), its baseline cw is fp32-maintained
    // anyway, and the fp32 noise is ~1e-4 of a row index — while the
    // fp64 weight conversions were what spilled ~143 dwords/lane in the
    // stream-K fused variants (cold-path scratch traffic ~1 GB/GEMM).
    //
    // Opaque copy of `sub`: everything derived from it (the FM*NREG
    // per-lane row weights below) is materialised INSIDE this cold block.
    // Without it the compiler hoists the loop-invariant weights into the
    // kernel prologue and keeps them live through the whole hot loop
    // (+68 VGPRs measured on the 64x64-wave tile -> spills on the bigger
    // tiles).
    //
    // A row weight is fm*MM + acc_row(reg, 0), a compile-time constant,
    // plus 4*sub.  The lane's part is turned into a float ONCE; each weight
    // is then one fp32 add of a literal — exact, all are integers below
    // 2^24, so the very float the integer sum + conversion gave and rw
    // keeps its bits — instead of an integer add and a conversion per term.
    int sub_o = sub;  // fresh opaque copy per fn: stops the
    asm volatile("" : "+v"(sub_o));  // weights being CSE'd+spilled
    const float row0 = (float)acc_row(0, sub_o);  // 4 * sub
    double colp = 0.0;
    float colwf = 0.f;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const float v = acc[fm][fn][reg];
        colp += (double)v;
        colwf = fmaf((float)(fm * MM + acc_row(reg, 0)) + row0, v, colwf);
      }
    const float rc =
        (float)(dslice_sum<MM>(colp) - (double)slice_sum<MM>(cc[fn]));
    const float rw = slice_sum<MM>(colwf) - slice_sum<MM>(cw[fn]);
    const bool cbad = fabsf(rc) > tau;
    const int row = (int)rintf(rw / (cbad ? rc : 1.f));
    if constexpr (LOG) {
      any_bad |= __any(cbad) != 0;
      const int lane = __lane_id();
      if (cbad && lane < MM) {  // one reporter per column
        const bool located = row >= 0 && row < FM * MM;
        const int slot = atomicAdd(ctx.log.counters + FLOG_N_EVENTS, 1);
        atomicAdd(ctx.log.counters +
                      (located ? FLOG_CORRECTED : FLOG_UNCORRECTED), 1);
        if (slot >= 0 && slot < ctx.log.capacity) {
          int* ev = ctx.log.events + (size_t)slot * FLOG_EVENT_DWORDS;
          ev[FLOG_EV_I] = located ? ctx.i0 + row : -1;
          ev[FLOG_EV_J] = ctx.j0 + fn * MM + lane;
          ev[FLOG_EV_K_BEGIN] = ctx.k_begin;
          ev[FLOG_EV_K_END] = ctx.k_end;
          ev[FLOG_EV_STATUS] =
              located ? FLOG_STATUS_CORRECTED : FLOG_STATUS_UNCORRECTED;
          ev[FLOG_EV_MAGNITUDE] = __float_as_int(rc);
          ev[FLOG_EV_BAND_ROW] = ctx.i0;
          ev[FLOG_EV_BAND_ROWS] = FM * MM;
        }
      }
    }
    int sub_c = sub;  // independent opaque copy for the correct pass
    asm volatile("" : "+v"(sub_c));
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      // a blended row outside [0, FM*MM) matches no fm: the fail-safe
      if (FM > 1 && !__any(cbad && row >= fm * MM && row < (fm + 1) * MM))
        continue;
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const bool hit = cbad && (fm * MM + acc_row(reg, sub_c) == row);
        acc[fm][fn][reg] -= hit ? rc : 0.f;
      }
    }
  }
  if constexpr (LOG) {
    if (!any_bad && __lane_id() == 0)
      atomicAdd(ctx.log.counters + FLOG_UNLOCATED, 1);
  }
}

// Segment-sum precompute: for a column-major MxK matrix, per SEG-row band,
// the plain column sum s = sum_{i in [seg*SEG, +SEG)} A[i + k*M] and the
// row-index-weighted sum w = sum_i (i % SEG) * A[i + k*M] used by the
// ratio locate (fault row = round(rw / rc)).  The pair is written
// INTERLEAVED — S[seg * 2*sstr + 2k] = s, S[seg * 2*sstr + 2k + 1] = w —
// so the fused kernel's encode fetches both with a single ds_read_b64 per
// k-step (the two separate b32 broadcast reads were one of the extra
// issue slots behind the tall tier's 21% fused overhead).
// One workgroup per column k, coalesced f32x4 sweep, SEG/4-lane shuffle
// groups, no LDS, no atomics.  sstr must be >= K and a multiple of 64 (the
// fused kernel streams 64-k strips with 4-B/lane global_load_lds pairs,
// never crossing rows).
template <int SEG>
__device__ __attribute__((always_inline)) inline void segsum_column(
    int M, int sstr, const float* __restrict__ A, float* __restrict__ S) {
  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  const float* col = A + (size_t)k * M;
  constexpr int GL = SEG / 4;  // lanes per segment group (4|8|16)
  for (int base = 0; base < M; base += 1024) {
    const int idx = base + tid * 4;
    float s = 0.f, w = 0.f;
    if (idx < M) {
      const f32x4 v = *(const f32x4*)(col + idx);
      s = (v[0] + v[1]) + (v[2] + v[3]);
      const float i0 = (float)(idx % SEG);
      w = i0 * v[0] + (i0 + 1.f) * v[1] + (i0 + 2.f) * v[2] +
          (i0 + 3.f) * v[3];
    }
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

template <int SEG>
__global__ __launch_bounds__(256) void segsum_kernel(
    int M, int K, int sstr, const float* __restrict__ A,
    float* __restrict__ S) {
  segsum_column<SEG>(M, sstr, A, S);
}

// Strided-batched twin, launched on a (K, nA) grid: blockIdx.y picks the
// matrix (strideA floats apart) and its copy of the per-matrix workspace
// layout (strideS floats apart).
template <int SEG>
__global__ __launch_bounds__(256) void segsum_batched_kernel(
    int M, int K, int sstr, const float* __restrict__ A,
    float* __restrict__ S, long long strideA, long long strideS) {
  const long long z = blockIdx.y;
  segsum_column<SEG>(M, sstr, A + z * strideA, S + z * strideS);
}

// ---------------------------------------------------------------------------
// Device building blocks shared by the classic kernel (sgemm_mfma, below),
// the stream-K kernel and its fixup pass (ft_streamk.hpp).  All are inlined
// into their callers; the kernels keep only their own work decomposition.
// ---------------------------------------------------------------------------

// Where one thread sits in its workgroup's tile: wave and lane, the lane's
// k-slice within one MFMA k-step (sub) and its row of the A fragment / column
// of the B fragment (r), and the wave tile's offset (wi0, wj0) in the block
// tile.
struct thread_pos {
  int tid, wave, lane, sub, r, wm_idx, wi0, wj0;
};

// Compile-time geometry of one tile configuration: thread layout, fragment
// counts and the LDS map.
template <int BM_, int BN_, int BK_, int WM_, int WN_, int MM_, bool ABFT>
struct tile_geom {
  using T = mfma_traits<MM_>;
  static constexpr int BM = BM_, BN = BN_, BK = BK_;
  static constexpr int WM = WM_, WN = WN_, MM = MM_;
  static constexpr int KSTEP = T::kstep;
  static constexpr int NREG = T::nreg;
  static constexpr int WAVES_M = BM / WM, WAVES_N = BN / WN;
  static constexpr int NWAVES = WAVES_M * WAVES_N;
  static constexpr int THREADS = NWAVES * 64;
  static constexpr int FM = WM / MM, FN = WN / MM;
  static constexpr int TPT = FM * FN * NREG;  // per-thread floats of one tile
  static constexpr int BUF = (BM + BN) * BK;  // floats per double-buffer half
  // ABFT checksum strips: per wave, a private [2 pair-buffers][sa(64) |
  // saw(64)] window of the precomputed segment sums, streamed by
  // global_load_lds.  Only A-side sums are needed: the column checksums
  // detect, the weighted ones locate the row, and the column is lane-local.
  static constexpr int STRIP_OFF = 2 * BUF;
  static constexpr int LDS_FLOATS =
      ABFT ? (STRIP_OFF + NWAVES * 256) : (2 * BUF);
  // A strip load covers 64 k values = PPS panels (one stream-K work unit);
  // strips are double buffered by strip-window parity.
  static constexpr int PPS = 64 / BK;
  static_assert(!ABFT || (BK <= 64 && 64 % BK == 0),
                "ABFT needs BK dividing 64");

  static __device__ inline thread_pos thread(int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    const int wm_idx = wave / WAVES_N, wn_idx = wave % WAVES_N;
    return {tid, wave, lane, lane / MM, lane % MM, wm_idx, wm_idx * WM,
            wn_idx * WN};
  }
  // this wave's strip buffer for 64-k windows of parity pb
  static __device__ inline float* strip(float* lds, int wave, int pb) {
    return &lds[STRIP_OFF + wave * 256 + pb * 128];
  }
};

// async HBM -> LDS copy of BYTES per lane.  The source address is PER-LANE;
// the LDS side is a wave-uniform base + lane * BYTES.
template <int BYTES>
__device__ __attribute__((always_inline)) inline void glds(const float* src,
                                                           float* dst) {
  const auto* s = (const __attribute__((address_space(1))) void*)src;
  auto* d = (__attribute__((address_space(3))) void*)dst;
  // the builtin takes its size as a literal only
  static_assert(BYTES == 16 || BYTES == 4);
  if constexpr (BYTES == 16)
    __builtin_amdgcn_global_load_lds(s, d, 16, 0, 0);
  else
    __builtin_amdgcn_global_load_lds(s, d, 4, 0, 0);
}

// Stages one ROWS x BK operand panel (rows row0.. of the column-major
// matrix g with leading dimension ld, columns k0..) into dst, LDS layout
// [k][row] with row contiguous, 16 B per lane.  Staging passes may be
// fractional in WHOLE WAVES (e.g. the fused tall twin at BKF=8 stages a
// 256-float B panel with a 128-thread block: 0 full passes + a 64-lane
// remainder by wave 0).
template <int ROWS, int BK, int THREADS>
__device__ __attribute__((always_inline)) inline void stage_operand(
    float* dst, const float* __restrict__ g, int ld, int row0, int k0, int tid,
    int wave) {
  constexpr int GF = (ROWS * BK) / (THREADS * 4);  // full dwordx4 passes
  constexpr int GR = (ROWS * BK / 4) % THREADS;    // remainder lanes
  static_assert(GR % 64 == 0, "stage remainder must be whole waves");
  static_assert(GF + GR > 0, "tile too small");
  auto pass = [&](int c0) __attribute__((always_inline)) {
    const int f = (c0 + tid) * 4;  // per-lane float index
    const int k = f / ROWS, i = f % ROWS;
    glds<16>(g + (row0 + i) + (size_t)(k0 + k) * ld,
             dst + (c0 + wave * 64) * 4);
  };
#pragma unroll
  for (int t = 0; t < GF; ++t) pass(t * THREADS);
  if constexpr (GR > 0) {
    if (tid < GR) pass(GF * THREADS);
  }
}

// ABFT strip staging: one 4-B/lane glds pair per TWO K panels.  Each wave
// streams its own 64-k window of the precomputed segment sums into its
// private LDS strip dst.  No extra barrier, no cooperative pass: the strips
// ride the same prefetch pipeline as the A/B panels and are drained by the
// same end-of-panel __syncthreads.
// Workspace layout (set up by the launcher): per WM-row band of A (segA),
// one row of 2*sstr floats with (plain, row-weighted) segment sums
// INTERLEAVED at [2k], [2k+1] — a 64-k window is 128 contiguous floats,
// fetched by two 64-lane glds loads (lane l fetches pair-element 2*k0 + l)
// and consumed with one ds_read_b64 per k-step.
__device__ __attribute__((always_inline)) inline void strip_stage(
    float* dst, const float* __restrict__ SA, int sstr, int segA, int k0,
    int lane) {
  const float* ga = SA + (size_t)segA * 2 * sstr + 2 * k0 + lane;
  glds<4>(ga, dst);
  glds<4>(ga + 64, dst + 64);
}

// ABFT verify / locate / correct of one wave tile: wave-autonomous,
// registers only.  Two-phase: the cheap detect (detect_partials: total tile
// sum vs total checksum) runs every verify window.  Its residual is
// identical across the wave's lanes, so the branch is uniform, and only a
// wave that actually absorbed a fault enters locate_correct(), which gets
// the detect's per-fn partials: the fault-free common case never pays for
// location.
//
// (i0_tile, j0_tile) is the block tile's first row / column and kbase its
// first k (0 in the classic kernel, the segment's start in stream-K); p_end
// is the window's end panel counted from kbase, and windows start at
// multiples of ppg panels.  These only feed the fault-log context, which is
// built in the cold branch: the window's first panel needs no register of
// its own in the loop.
template <class G, bool LOG>
__device__ __attribute__((always_inline)) inline void verify_window(
    typename G::T::acc_t (&acc)[G::FM][G::FN], const checksum_regs<G::FN>& cs,
    int sub, float tau, const FaultLog& flog, int i0_tile, int j0_tile,
    int kbase, int p_end, int ppg) {
  constexpr int FM = G::FM, FN = G::FN, MM = G::MM;
  float cc[FN], cw[FN], p[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    cc[fn] = cs.cc(fn);
    cw[fn] = cs.cw(fn);
  }
  const float res = detect_partials<FM, FN, MM>(acc, cc, p);
  if (__builtin_expect(fabsf(res) > tau, 0)) {
    FaultCtx ctx;
    if constexpr (LOG) {
      ctx.log = flog;
      const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      ctx.i0 = i0_tile + (wv / G::WAVES_N) * G::WM;
      ctx.j0 = j0_tile + (wv % G::WAVES_N) * G::WN;
      ctx.k_begin = kbase + ((p_end - 1) / ppg) * ppg * G::BK;
      ctx.k_end = kbase + p_end * G::BK;
    }
    locate_correct<FM, FN, MM, LOG>(acc, cc, cw, p, sub, tau, ctx);
  }
}

// Strides of a strided-batched launch, in floats: entry z of the batch reads
// A + z * A, B + z * B and SA + z * SA and writes C + z * C.  A stride of 0
// shares one operand (and its segment sums) between all entries.
struct BatchStrides {
  long long A = 0, B = 0, C = 0, SA = 0;
};

// BATCHED: one GEMM per blockIdx.z (launch_tier_batched).  Only the prologue
// knows: it moves the operand pointers, and the fault log to the entry's own
// (counters[z], events[z]) of a batch-major log array, by wave-uniform 64-bit
// offsets.  Everything below it is the single-matrix kernel, so an entry's C
// has the bits of a single launch on the same operands.  The unbatched
// instantiations never look at bs.
template <int BM, int BN, int BK, int WM, int WN, int MM, bool ABFT,
          bool INJECT, int OCC = 2, bool LOG = false, bool BATCHED = false>
__global__ __launch_bounds__(
    (tile_geom<BM, BN, BK, WM, WN, MM, ABFT>::THREADS), OCC) void sgemm_mfma(
    int M, int N, int K, const float* __restrict__ A,
    const float* __restrict__ B, float* __restrict__ C, float alpha,
    float beta, int verify_iters, int inject_stride, float tau, float inj_mag,
    const float* __restrict__ SA, int sstr, FaultLog flog, BatchStrides bs) {
  using G = tile_geom<BM, BN, BK, WM, WN, MM, ABFT>;
  if constexpr (BATCHED) {
    const long long z = blockIdx.z;
    A += z * bs.A;
    B += z * bs.B;
    C += z * bs.C;
    if constexpr (ABFT) SA += z * bs.SA;
    if constexpr (LOG) {
      flog.counters += z * FLOG_N_COUNTERS;
      flog.events += z * flog.capacity * FLOG_EVENT_DWORDS;
    }
  }
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

  auto stage = [&](int q, int k0) __attribute__((always_inline)) {
    stage_operand<BM, BK, THREADS>(&lds[q * BUF], A, M, im0, k0, tid, wave);
    stage_operand<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B, N, jn0, k0, tid,
                                   wave);
  };

  const int segA = bx * G::WAVES_M + wm_idx;  // this wave's WM-row band of A
  auto stage_strip = [&](int pb, int k0) __attribute__((always_inline)) {
    strip_stage(G::strip(lds, wave, pb), SA, sstr, segA, k0, lane);
  };

  // ---- ABFT scheme (verify_window -> locate_correct, above) ----
  // Ratio locate: the fault's COLUMN is lane-local (acc column == lane's
  // r), its magnitude is the column residual rc; its ROW index is
  // round(rw / rc) where rw is the residual of the row-index-WEIGHTED
  // column checksum.  This replaces the reference's row x column residual
  // intersection (ft_sgemm_huge.cuh:422-485) whose row residuals needed a
  // full cross-lane butterfly per accumulator register — the measured
  // window cost dropped ~10x because no row reductions exist at all.
  //
  // Guarantee (same as the reference): ONE fault per verify window per
  // wave tile.  TWO faults e1 at row r1 and e2 at row r2 landing in the
  // SAME column of one wave tile within one window degrade differently
  // from the reference: rc = e1 + e2, row = round((r1*e1 + r2*e2) /
  // (e1+e2)), and rc is subtracted IF some accumulator row matches that
  // blended index — correcting a clean element by the combined magnitude
  // (the reference's intersection scheme instead corrects every
  // row-candidate x col-candidate).  When the blend rounds outside the
  // fragment's row range nothing matches and the kernel fail-safes to
  // detected-but-uncorrected.  Faults in different columns (the common
  // double-fault shape) locate independently per lane and correct fine.
  // Bursts start at multiples of verify_iters panels, from k = 0.
  auto verify = [&](int it_end) __attribute__((always_inline)) {
    verify_window<G, LOG>(acc, cs, sub, tau, flog, im0, jn0, 0, it_end,
                          verify_iters);
  };

  // ---- main K loop: one barrier per BK panel, glds prefetch overlaps ----
  // Structure: bursts of `verify_iters` panels.  The inner panel loop never
  // touches the accumulator with VALU code; injection and verify/correct
  // run at burst boundaries only (a conditional VALU read of acc inside the
  // panel loop makes hipcc shuttle the whole accumulator file through VGPR
  // copies every panel — measured 2x wall time on the huge tier).
  stage(0, 0);
  if constexpr (ABFT) stage_strip(0, 0);  // window 0 (panels 0..PPS-1)
  FT_PARA_SYNC();
  __syncthreads();  // drains in-flight glds

  const int niter = K / BK;
  int it = 0;
  while (it < niter) {
    if constexpr (INJECT) {
      // Deterministic rotating injector, once per verify window (reference:
      // ft_sgemm_huge.cuh:324-327 injects in every block with a rotating
      // thread id; here the victim also rotates across waves).
      if (tid == ((unsigned)(it / inject_stride) * 67u) % THREADS)
        acc[0][0][0] += inj_mag;
    }
    const int burst_end = (it + verify_iters < niter) ? it + verify_iters
                                                      : niter;
    for (; it < burst_end; ++it) {
      const int q = it & 1;
      if (it + 1 < niter) {
        stage(q ^ 1, (it + 1) * BK);
        // a new strip window rides along every PPS-th panel prefetch
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
      // Encode (reference encode: ft_sgemm_huge.cuh:150-213, redesigned
      // around the offline segsum pass + ratio locate): per k-slice ONE
      // ds_read_b64 fetches the interleaved (plain, row-weighted)
      // segment-sum pair, and cs.encode() adds its two fmas per B fragment.
      // Where a k-step has more than one MFMA (defer_encode) the fused loop
      // keeps the plain loop's LDS wait structure: the strip reads only
      // PARK their pair next to the B fragments (which stay in registers
      // until the panel's last MFMA anyway) and the encode runs as one
      // block BEHIND the panel barrier, in the shadow of the MFMAs the
      // compiler sinks there.  With the fmas next to the reads, LDS
      // returning in order forced a full lgkmcnt(0) drain per k-step.  A
      // source reorder alone is undone by the scheduler; the empty asm on
      // the pairs, ordered after the barrier, is what pins it
      // (docs/ABLATION.md §5b).  Per lane the fmas into each checksum
      // still run in ascending k: bit-identical.
      // This panel body and the alpha/beta epilogue below are written out
      // again in ft_streamk.hpp: as shared functions they changed register
      // counts or the epilogue's rounding (docs/ABLATION.md §5e).
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

        // interleave VMEM/DS/MFMA scheduling groups (+1% measured)
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

  // ---- epilogue: alpha/beta merge, float4 along column-major columns ----
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int j = jn0 + wj0 + fn * MM + r;
      float* colbase = C + (size_t)j * M + im0 + wi0 + fm * MM;
#pragma unroll
      for (int g = 0; g < G::NREG / 4; ++g) {
        float* p = colbase + 4 * sub + 8 * g;
        f32x4 out;
        if (beta != 0.f) {
          const f32x4 prev = *(const f32x4*)p;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            out[u] = alpha * acc[fm][fn][4 * g + u] + beta * prev[u];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) out[u] = alpha * acc[fm][fn][4 * g + u];
        }
        *(f32x4*)p = out;
      }
    }
}

}  // namespace ftsgemm
