// ft_ragged_grouped_streamk.hpp — stream-K for the grouped ragged launch: the
// work walk of sgemm_mfma_ragged_streamk (ft_ragged_streamk.hpp) over the
// units of all entries of a GroupedArgs, with the descriptor table of the
// classic grouped launch (ft_ragged.hpp, GROUPED; grouped_table.h).  Compiled
// in its own translation units
// (csrc/generated/kernel_<tier>_ragged_gsk_{nn,tn,nt,tt}.hip): neither
// the single-launch stream-K kernels nor the classic grouped ones change.
//
// Why: the classic grouped launch runs one workgroup per output tile.  The
// product it was built for, the grad_weight of a mixture-of-experts layer
// (M = in, N = out, K = tokens of the expert), has few, fixed tiles and a
// deep K that differs per expert: the chip is half idle and the launch is as
// long as its deepest expert.  Here the work is the list of
//   total = sum_e tiles_e * upt_e,   upt_e = max(1, ceil(K_e / 64))
// units, ordered by entry, then tile (bx fastest, as the classic grouped
// grid), then k, cut into G balanced contiguous ranges, one per workgroup.
// One cut over the units of all entries evens out a deep expert next to a
// shallow one, which no loop of single stream-K launches can.
//
// The max(1, ...) gives an entry with K_e == 0 (an expert without tokens) one
// empty unit per tile: its owner runs no panel and takes the guarded
// epilogue, which writes beta * C (exact zeros, C not read, for beta == 0).
// Such an entry has no workspace region and its strip prefetch is skipped,
// as in the classic grouped kernel; no operand is dereferenced (every staging
// lane fails k < K and reads ragged_zero_word).  Entries with M_e == 0 or
// N_e == 0 have no units and are never looked up.
//
// A workgroup's range may cross tile and entry boundaries.  At each segment
// start it finds its entry in the table's unit-start prefix (GroupSkTable),
// by binary search for its first segment and by advancing thereafter, and,
// when the entry changed, loads the descriptor over its working M, N, K,
// leading dimensions, pointers, fast bits, sstr, workspace offset, verify
// stride and log slot, every load through uniform() so that the descriptor
// lives in SGPRs.  Below that the segment body is sgemm_mfma_ragged_streamk's,
// written out again, and slots, fixup order and ABFT composition are as
// documented there: head partial in slot 2*wg, tail in 2*wg + 1 (a workgroup
// has at most one of each, entry boundaries included, because only its first
// segment can start inside a tile and only its last can end inside one), the
// fixup pass sums the first owner's tail and the following workgroups' heads
// in workgroup order; no atomics, no flags, no residency assumption.

#pragma once

#include "ft_ragged_streamk.hpp"

namespace ftsgemm {

// Units per tile of an entry with depth K: 64-k windows, one (empty) for
// K == 0.
__host__ __device__ inline int grouped_sk_upt(int K) {
  const int w = (K + 63) >> 6;
  return w < 1 ? 1 : w;
}

// sk_fixup_ragged_kernel for a grouped launch: one workgroup per tile of all
// entries (the classic grouped grid).  The tile's global unit range comes
// from unit_start; a tile one workgroup owns whole, every K == 0 tile among
// them, was written by the main kernel and exits at once.
template <int BM, int BN, int WM, int WN, int MM>
static __global__ __launch_bounds__(
    (tile_geom<BM, BN, 64, WM, WN, MM, false>::THREADS))
void sk_fixup_ragged_grouped_kernel(int nwg, float alpha, float beta,
                                    const float* __restrict__ partials,
                                    GroupTable gt, GroupSkTable sk) {
  using G = tile_geom<BM, BN, 64, WM, WN, MM, false>;
  const int e = grouped_entry_of(gt, blockIdx.x);
  const GroupedEntry& d = gt.entry[e];
  const int tile = blockIdx.x - uniform(gt.tile_start[e]);
  const int upt = grouped_sk_upt(uniform(d.K));
  const int total = uniform(sk.unit_start[gt.groups]);
  const int u0 = uniform(sk.unit_start[e]) + tile * upt;
  const int q = total / nwg, rem = total % nwg;
  const int g0 = sk_wg_of_unit(u0, q, rem);
  const int gl = sk_wg_of_unit(u0 + upt - 1, q, rem);
  if (g0 == gl) return;  // fully owned -> already epilogued

  const thread_pos t = G::thread(threadIdx.x);
  float s[G::TPT];
  load_partial<G, false>(s, partial_slot<G>(partials, 2 * g0 + 1, t.tid));
  for (int gc = g0 + 1; gc <= gl; ++gc)
    load_partial<G, true>(s, partial_slot<G>(partials, 2 * gc, t.tid));
  const int ntm = uniform(d.tiles_x);
  float* C = uniform(d.C);
  const bool c_vec =
      (uniform(d.fast) & RAGGED_FAST_C) && ((uintptr_t)C & 15) == 0;
  ragged_epilogue<G>(s, t, (tile % ntm) * BM, (tile / ntm) * BN, uniform(d.M),
                     uniform(d.N), uniform(d.ldc), c_vec, alpha, beta, C);
}

// The grouped ragged stream-K kernel, on dim3(G) workgroups.  SA0 and flog0
// are the launch's workspace and first log; the entry's own are derived at
// each entry change.
template <int BM, int BN, int BK, int WM, int WN, int MM, bool ABFT,
          bool INJECT, int OCC = 2, bool LOG = false, bool TA = false,
          bool TB = false>
__global__ __launch_bounds__(
    (tile_geom<BM, BN, BK, WM, WN, MM, ABFT>::THREADS),
    OCC) void sgemm_mfma_ragged_grouped_streamk(float alpha, float beta,
                                                float tau, float inj_mag,
                                                const float* __restrict__ SA0,
                                                float* __restrict__ partials,
                                                FaultLog flog0, GroupTable gt,
                                                GroupSkTable sk) {
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

  // balanced contiguous unit ranges over the units of all entries: the first
  // (total % gridDim.x) workgroups take one extra unit
  const int total = uniform(sk.unit_start[gt.groups]);
  const int wg = blockIdx.x;
  const int q = total / gridDim.x, rem = total % gridDim.x;
  int u = wg * q + (wg < rem ? wg : rem);
  const int u_end = u + q + (wg < rem ? 1 : 0);

  // the segment's entry: what the classic grouped prologue loads, reloaded
  // when the walk enters another entry; all workgroup-uniform
  int M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0, fast = 0, sstr = 0,
      istride = 1, ntm = 1, upt = 1;
  const float* A = nullptr;
  const float* B = nullptr;
  float* C = nullptr;
  const float* SA = SA0;
  FaultLog flog = flog0;
  int ent = -1, e_begin = 0, e_end = 0;  // units [e_begin, e_end) are ent's

  // the segment's tile; all workgroup-uniform, set at each segment start
  int im0 = 0, jn0 = 0, segA = 0;
  bool a_fast = false, b_fast = false, band_real = false;

  using StA = stage_operand_t<BM, BK, THREADS>;
  using StB = stage_operand_t<BN, BK, THREADS>;
  typename StA::regs ra;  // a transposed operand's next panel (fast path)
  typename StB::regs rb;
  constexpr bool SPLIT = TA && TB;   // ft_ragged.hpp says why
  constexpr bool LATE_A = TA && !TB;  // ft_ragged_streamk.hpp says why

  // stage / stage_mid / stage_finish of sgemm_mfma_ragged_streamk, written
  // out again
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

  while (u < u_end) {
    // ---- the segment's entry ----
    if (u >= e_end) {
      int e;
      if (ent < 0) {
        // first segment: the last e with unit_start[e] <= u (entries without
        // units share their successor's start and are never returned)
        e = grouped_entry_of(GroupTable{sk.unit_start, gt.entry, gt.groups},
                             u);
      } else {
        e = ent + 1;
        while (u >= uniform(sk.unit_start[e + 1])) ++e;
      }
      ent = e;
      e_begin = uniform(sk.unit_start[e]);
      e_end = uniform(sk.unit_start[e + 1]);
      const GroupedEntry& d = gt.entry[e];
      M = uniform(d.M), N = uniform(d.N), K = uniform(d.K);
      lda = uniform(d.lda), ldb = uniform(d.ldb), ldc = uniform(d.ldc);
      A = uniform(d.A), B = uniform(d.B), C = uniform(d.C);
      fast = ragged_fast_entry(uniform(d.fast), A, B, C);
      ntm = uniform(d.tiles_x);
      upt = grouped_sk_upt(K);
      if constexpr (ABFT) {
        sstr = uniform(d.sstr);
        SA = SA0 + uniform(d.ws_off);
        istride = uniform(sk.istride[e]);
      }
      if constexpr (LOG) {
        flog.counters = flog0.counters + (long long)e * FLOG_N_COUNTERS;
        flog.events =
            flog0.events + (long long)e * flog0.capacity * FLOG_EVENT_DWORDS;
      }
    }

    const int lu = u - e_begin;
    const int tile = lu / upt;  // entry-local
    const int w_lo = lu - tile * upt;
    const int seg_units = (u_end - u < upt - w_lo) ? (u_end - u)
                                                   : (upt - w_lo);
    const int w_hi = w_lo + seg_units;
    const int by = tile / ntm, bx = tile - by * ntm;
    im0 = bx * BM, jn0 = by * BN;
    segA = bx * G::WAVES_M + wm_idx;
    band_real = segA * WM < M;
    a_fast = (fast & RAGGED_FAST_A) && im0 + BM <= M;
    b_fast = (fast & RAGGED_FAST_B) && jn0 + BN <= N;
    const int kbase = w_lo << 6;
    const int kend = (w_hi << 6) < K ? (w_hi << 6) : K;
    const int npan = (kend - kbase + BK - 1) / BK;  // 0 for a K == 0 unit

    // behind the previous segment's closing barrier: both buffers are free
    stage(0, kbase);
    stage_mid(0, kbase);
    stage_finish(0, kbase);
    if constexpr (ABFT) {
      // an entry with K == 0 has no sums (no workspace region)
      if (K > 0) stage_strip(w_lo & 1, kbase);
    }
    FT_PARA_SYNC();
    __syncthreads();

    const int PPG = istride * PPS;  // panels per inject+verify group
    int p = 0;
    while (p < npan) {
      if constexpr (INJECT) {
        // deterministic rotating victim per (entry-local tile, unit group)
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
                for (int e4 = 0; e4 < 4; ++e4)
                  if (i + e4 < M) prev[e4] = p4[e4];
              }
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4)
                out[e4] = alpha * acc[fm][fn][4 * g4 + e4] + beta * prev[e4];
            } else {
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4)
                out[e4] = alpha * acc[fm][fn][4 * g4 + e4];
            }
            if (whole) {
              *(f32x4*)p4 = out;
            } else {
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4)
                if (i + e4 < M) p4[e4] = out[e4];
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
auto ragged_grouped_streamk_variant(const GroupedArgs& g, bool logged) {
  return select_variant(
      g.abft, g.inject, logged,
      &sgemm_mfma_ragged_grouped_streamk<BM, BN, BK, WM, WN, MM, false, false,
                                         2, false, TA, TB>,
      [](auto inj, auto lg) {
        return &sgemm_mfma_ragged_grouped_streamk<
            BM, BN, BKF, WM, WN, MM, true, decltype(inj)::value, 2,
            decltype(lg)::value, TA, TB>;
      });
}

// Workgroups per CU of the variant g selects, always the unlogged one (the
// rule of ragged_streamk_occupancy).  0 when the query fails.  Launches
// nothing.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false>
int ragged_grouped_streamk_occupancy(const GroupedArgs& g) {
  constexpr int THREADS = tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS;
  int maxblk = 0;
  const auto kfn =
      ragged_grouped_streamk_variant<BM, BN, BK, BKF, WM, WN, MM, TA, TB>(
          g, false);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &maxblk, (const void*)kfn, THREADS, 0) != hipSuccess)
    return 0;
  return maxblk > 0 ? maxblk : 0;
}

// Grouped stream-K launch of one tier on g.sk_grid workgroups (clamped to the
// unit count): the grouped encode of launch_tier_ragged_grouped unchanged,
// the main kernel, the fixup pass over the tiles of all entries.  g.table
// holds the stream-K section (grouped_table_build with sk_grid > 0).  Checks
// nothing (sgemm_grouped_launch does).  No allocation, no copy, no sync, no
// environment lookup and no mempool call: the launch can be captured.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false>
hipError_t launch_tier_ragged_grouped_streamk(const GroupedArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  long long tiles = 0, total = 0;
  int max_sstr = 0, max_bands = 0;
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    const long long te =
        (long long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    tiles += te;
    total += te * grouped_sk_upt(p.K);
    if (p.M > 0 && p.N > 0 && p.K > 0) {
      const int sstr = abft_sstr(p.K), bands = (p.M + WM - 1) / WM;
      if (sstr > max_sstr) max_sstr = sstr;
      if (bands > max_bands) max_bands = bands;
    }
  }
  if (tiles == 0) return hipSuccess;  // every entry is empty
  const int G = g.sk_grid < total ? g.sk_grid : (int)total;
  const GroupTable gt = grouped_table_view(g.table, g.groups);
  const GroupSkTable sk = grouped_sk_table_view(g.table, g.groups);
  const int egroups = g.groups < 65535 ? g.groups : 65535;
  if (abft && max_sstr > 0) {
    RoctxRange rr("abft_encode_segsum_ragged_grouped");
    if constexpr (TA) {
      const int kblocks = (max_sstr + 255) / 256;
      hipLaunchKernelGGL((segsum_ragged_t_kernel<WM, false, true>),
                         dim3(max_bands, kblocks < 1024 ? kblocks : 1024,
                              egroups),
                         dim3(256), 0, g.stream, 0, 0, 0, 0, nullptr, g.ws, 0LL,
                         0LL, gt);
    } else {
      hipLaunchKernelGGL((segsum_ragged_kernel<WM, false, true>),
                         dim3(max_sstr, egroups), dim3(256), 0, g.stream, 0, 0,
                         0, 0, nullptr, g.ws, 0LL, 0LL, gt);
    }
  }
  RoctxRange rr_main(abft ? (inject ? "ft_sgemm_ragged_grouped_streamk_abft_inject"
                                    : "ft_sgemm_ragged_grouped_streamk_abft")
                          : "sgemm_ragged_grouped_streamk_plain");
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn =
      ragged_grouped_streamk_variant<BM, BN, BK, BKF, WM, WN, MM, TA, TB>(
          g, flog.counters != nullptr);
  constexpr int THREADS = tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS;
  hipLaunchKernelGGL(kfn, dim3(G), dim3(THREADS), 0, g.stream, g.alpha, g.beta,
                     g.tau, g.inj_mag, (const float*)g.ws, g.sk_partials, flog,
                     gt, sk);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  // combine split tiles (fully-owned tiles exit immediately)
  hipLaunchKernelGGL((sk_fixup_ragged_grouped_kernel<BM, BN, WM, WN, MM>),
                     dim3((unsigned)tiles), dim3(THREADS), 0, g.stream, G,
                     g.alpha, g.beta, (const float*)g.sk_partials, gt, sk);
  return hipGetLastError();
}

}  // namespace ftsgemm
