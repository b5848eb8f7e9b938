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
// Transposed operands (template flags TA / TB, GemmArgs::transA / transB): a
// row-major operand, element (row, k) at g[k + row*ld], is a third way to fill
// the same [k][row] LDS panel.  stage_operand_guarded_t is the always-legal
// 4-B form; stage_operand_t is the fast one (16 B per lane along k into
// registers, transposed into LDS with 4-B writes after the panel's MFMA
// loop).  Everything after the staging is shared, so a transposed call has
// the bits of the plain call on the transposed copy.  The TA = TB = false
// instantiations are the kernels as they were and keep their own translation
// units; the others live in kernel_<tier>_ragged_{tn,nt,tt}.hip.
//
// Strided batches (template flag BATCHED, GemmArgs::batch > 1): the entry is
// blockIdx.z and, as in sgemm_mfma, only the prologue knows.  It moves A, B,
// C, SA and the fault log to entry z by wave-uniform 64-bit offsets
// (BatchStrides); everything below it is the single-product kernel, so entry
// z has the bits of the single launch on its views.  No stride has to be a
// multiple of 4, so entry z's base X + z*strideX can be misaligned where
// entry 0's is not.  The fast bits are therefore settled per entry: the host
// sets a bit from the leading dimension alone (ld % 4 == 0) and the prologue
// clears it unless the entry's own moved pointer is 16-B aligned.  That is
// two scalar ANDs per operand, it keeps the 16-B paths for every entry that
// can take them (with an odd stride, every fourth), and the other way —
// clearing the bit for the whole launch — would put every entry of such a
// batch on the 4-B paths.  Either is correct: the result does not depend on
// which staging ran.  The segment-sum kernels take the entry as one more grid
// dimension and test `vec` on the entry's own column pointer.  The
// BATCHED = false instantiations never look at the strides and keep their
// translation units; the batched ones live in
// kernel_<tier>_ragged_batched_{nn,tn,nt,tt}.hip.
//
// Grouped launches (template flag GROUPED, GroupedArgs): a list of products,
// each with its own M, N, K, leading dimensions and pointers, in one launch.
// The grid is one-dimensional over the tiles of all entries and the kernel
// takes a descriptor table (grouped_table.h).  Again only the prologue knows:
// it finds the block's entry by a binary search of blockIdx.x in the table's
// tile-start prefix (workgroup-uniform), derives (bx, by) inside the entry
// with bx fastest, as the two-dimensional grid orders them, and loads the
// entry's sizes, leading dimensions, pointers, window stride, workspace
// region and log slot over the kernel arguments of the same names; the fast
// bits are settled from the entry's own pointers as in a batch.  Below it
// runs the single-product kernel, so entry e has the bits, fault events
// included, of the single launch on its operands.  An entry with K == 0 runs
// no panel: its accumulators stay zero, the epilogue writes beta * C, and the
// one access that does not depend on the panel loop, the strip prefetch of
// window 0, is skipped (such an entry has no workspace).  The segment-sum
// kernels take the entry from a grid dimension sized for the largest entry
// and leave early where an entry is smaller (docs/ABLATION.md has the
// alternative).  The GROUPED = false instantiations never look at the table
// and keep their translation units; the grouped ones live in
// kernel_<tier>_ragged_grouped_{nn,tn,nt,tt}.hip.
//
// Classic decomposition only; the stream-K twin of the single launch is
// ft_ragged_streamk.hpp.

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

// The bits of `fast` that entry pointers A, B, C still allow (batched
// prologue; workgroup-uniform).
__device__ __attribute__((always_inline)) inline int ragged_fast_entry(
    int fast, const float* A, const float* B, const float* C) {
  if ((uintptr_t)A & 15) fast &= ~RAGGED_FAST_A;
  if ((uintptr_t)B & 15) fast &= ~RAGGED_FAST_B;
  if ((uintptr_t)C & 15) fast &= ~RAGGED_FAST_C;
  return fast;
}

// A value every lane of the workgroup holds alike, marked so: what a grouped
// prologue loads from the table decides workgroup-uniform branches and the
// LDS side of global_load_lds below.
__device__ __attribute__((always_inline)) inline int uniform(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __attribute__((always_inline)) inline long long uniform(
    long long x) {
  const unsigned long long v = (unsigned long long)x;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
template <class P>
__device__ __attribute__((always_inline)) inline P* uniform(P* p) {
  return (P*)uniform((long long)p);
}

// The entry that owns tile `tile` of a grouped launch: the last e with
// tile_start[e] <= tile.  Entries without tiles share their successor's
// start and are never returned.  tile < tile_start[groups].
__device__ __attribute__((always_inline)) inline int grouped_entry_of(
    const GroupTable& gt, int tile) {
  int lo = 0, hi = gt.groups;  // tile_start[lo] <= tile < tile_start[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (gt.tile_start[mid] <= tile)
      lo = mid;
    else
      hi = mid;
  }
  return uniform(lo);
}

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

// stage_operand_guarded for a transposed (row-major) operand: element
// (row i, k) is at g[k + i*ld].  The same lane -> (k, row) map and the same
// LDS image; consecutive lanes are ld floats apart in memory, so it is slow.
// It serves unaligned operands, edge blocks and the K tail.
template <int ROWS, int BK, int THREADS>
__device__ __attribute__((always_inline)) inline void stage_operand_guarded_t(
    float* dst, const float* __restrict__ g, int ld, int rows, int K, int row0,
    int k0, int tid, int wave) {
  static_assert((ROWS * BK) % THREADS == 0, "whole 4-B passes");
  constexpr int NP = (ROWS * BK) / THREADS;
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int f = t * THREADS + tid;
    const int k = k0 + f / ROWS, i = row0 + f % ROWS;
    const float* src =
        (i < rows && k < K) ? g + k + (size_t)i * ld : ragged_zero_word;
    glds<4>(src, dst + t * THREADS + wave * 64);
  }
}

// Which lane of a pass loads which 16-B quad (row, kq) of a transposed panel.
// FT_TRANS_ROW_FASTEST unset (shipped): the BK/4 quads of a row sit in
// consecutive lanes, so a wave reads whole 4*BK-byte row segments; the four
// 4-B LDS writes of a lane then go to bank row % 32 and are (BK/4)-way
// conflicted when ROWS is a multiple of 32.  Set: row fastest, conflict-free
// LDS writes, but the quads of one row segment are ROWS lanes apart.
// docs/ABLATION.md section 16 has both measured.
#ifdef FT_TRANS_ROW_FASTEST
constexpr bool kTransRowFastest = true;
#else
constexpr bool kTransRowFastest = false;
#endif

// Fast staging of a transposed operand, legal when the operand is 16-B
// aligned with ld % 4 == 0, the block's ROWS rows all exist and the panel is a
// whole one: load() reads 16 B per lane along k into registers
// (global_load_dwordx4), store() writes their transpose into the [k][row]
// panel with 4-B LDS writes — the image stage_operand leaves for the same
// values.  global_load_lds cannot do this (its LDS side is lane-linear).
// Passes may be fractional in whole waves, as in stage_operand.
template <int ROWS, int BK, int THREADS>
struct stage_operand_t {
  static constexpr int QPR = BK / 4;        // 16-B quads per row
  static constexpr int NQ = ROWS * QPR;     // quads per panel
  static constexpr int GF = NQ / THREADS;   // full passes
  static constexpr int GR = NQ % THREADS;   // remainder lanes
  static constexpr int NP = GF + (GR > 0 ? 1 : 0);
  static_assert(BK % 4 == 0, "16-B reads along k");
  static_assert(GR % 64 == 0, "stage remainder must be whole waves");
  static_assert(NP > 0, "tile too small");
  using regs = f32x4[NP];

  static __device__ __attribute__((always_inline)) inline void quad(
      int c, int& row, int& kq) {
    if constexpr (kTransRowFastest) {
      row = c % ROWS, kq = c / ROWS;
    } else {
      kq = c % QPR, row = c / QPR;
    }
  }
  static __device__ __attribute__((always_inline)) inline void load(
      regs& v, const float* __restrict__ g, int ld, int row0, int k0,
      int tid) {
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      if (t < GF || tid < GR) {
        int row, kq;
        quad(t * THREADS + tid, row, kq);
        v[t] = *(const f32x4*)(g + (k0 + 4 * kq) + (size_t)(row0 + row) * ld);
      }
    }
  }
  static __device__ __attribute__((always_inline)) inline void store(
      const regs& v, float* dst, int tid) {
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      if (t < GF || tid < GR) {
        int row, kq;
        quad(t * THREADS + tid, row, kq);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[(4 * kq + u) * ROWS + row] = v[t][u];
      }
    }
  }
};

// The sums of four consecutive rows that both segment-sum kernels combine:
// plain (v0+v1)+(v2+v3) and row-weighted with i0 = the first row's index in
// its band.  One function, so that contraction into fmas is decided once and
// the two kernels give the same bits.
__device__ __attribute__((always_inline)) inline void segsum_rows4(
    const f32x4& v, float i0, float& s, float& w) {
  s = (v[0] + v[1]) + (v[2] + v[3]);
  w = i0 * v[0] + (i0 + 1.f) * v[1] + (i0 + 2.f) * v[2] + (i0 + 3.f) * v[3];
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
// BATCHED: launched on (sstr, nA); blockIdx.y picks the matrix (strideA floats
// apart) and its copy of the workspace layout (strideS floats apart).  The
// sums, their order, the zero fill and the vec test (on the entry's own
// column) are the unbatched kernel's, which never looks at the strides.
// GROUPED: launched on (largest sstr, entries up to 65535); blockIdx.y walks
// the table's entries in steps of gridDim.y and a block beyond its entry's
// sstr, or of an entry without workspace, does nothing.
template <int SEG>
__device__ __attribute__((always_inline)) inline void segsum_ragged_column(
    int M, int K, int lda, int sstr, const float* __restrict__ A,
    float* __restrict__ S, int k, int tid) {
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
    float s, w;
    segsum_rows4(v, (float)(idx % SEG), s, w);
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

// Does entry e of a grouped launch have segment sums (a workspace region)?
__device__ __attribute__((always_inline)) inline bool grouped_has_sums(
    const GroupedEntry& e) {
  return e.M > 0 && e.N > 0 && e.K > 0;
}

template <int SEG, bool BATCHED = false, bool GROUPED = false>
__global__ __launch_bounds__(256) void segsum_ragged_kernel(
    int M, int K, int lda, int sstr, const float* __restrict__ A,
    float* __restrict__ S, long long strideA, long long strideS,
    GroupTable gt) {
  if constexpr (GROUPED) {
    for (int e = blockIdx.y; e < gt.groups; e += gridDim.y) {
      const GroupedEntry& d = gt.entry[e];
      if (!grouped_has_sums(d) || (int)blockIdx.x >= d.sstr) continue;
      segsum_ragged_column<SEG>(d.M, d.K, d.lda, d.sstr, d.A, S + d.ws_off,
                                blockIdx.x, threadIdx.x);
    }
    return;
  }
  if constexpr (BATCHED) {
    const long long z = blockIdx.y;
    A += z * strideA;
    S += z * strideS;
  }
  segsum_ragged_column<SEG>(M, K, lda, sstr, A, S, blockIdx.x, threadIdx.x);
}

// Plain and weighted sums of rows [4*g0, 4*(g0+NG)) of one band at one k of a
// transposed A: the 4-row sums of segsum_rows4 combined by the balanced
// pairwise tree that segsum_ragged_kernel's xor butterfly forms (lane 0 of a
// group adds, level by level, the sum of the next 1, 2, 4, ... lanes).
template <int NG>
__device__ __attribute__((always_inline)) inline void segsum_t_tree(
    const float* __restrict__ p, size_t lda, int row0, int g0, int M, float& s,
    float& w) {
  if constexpr (NG == 1) {
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    const int i = row0 + 4 * g0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u < M) v[u] = p[(size_t)(i + u) * lda];
    segsum_rows4(v, (float)(4 * g0), s, w);
  } else {
    float s1, w1;
    segsum_t_tree<NG / 2>(p, lda, row0, g0, M, s, w);
    segsum_t_tree<NG / 2>(p, lda, row0, g0 + NG / 2, M, s1, w1);
    s += s1;
    w += w1;
  }
}

// segsum_ragged_kernel for a transposed A (element (i, k) at A[k + i*lda]):
// the same workspace, the same zero fill of [K, sstr) and the same bits.
// Threads run along k, so the reads are coalesced; blockIdx.x is the band and
// each thread walks its band's SEG rows.  Rows >= M contribute exact zeros.
// BATCHED: blockIdx.z picks the matrix and its workspace copy, as above.
// GROUPED: launched on (most bands, k blocks of the largest sstr, entries up
// to 65535); blockIdx.z walks the table's entries in steps of gridDim.z, and
// a block beyond its entry's bands does nothing.
template <int SEG>
__device__ __attribute__((always_inline)) inline void segsum_ragged_t_band(
    int M, int K, int lda, int sstr, const float* __restrict__ A,
    float* __restrict__ S, int band) {
  float* out = S + (size_t)band * 2 * sstr;
  for (int k = blockIdx.y * 256 + threadIdx.x; k < sstr;
       k += gridDim.y * 256) {
    float s = 0.f, w = 0.f;
    if (k < K) segsum_t_tree<SEG / 4>(A + k, (size_t)lda, band * SEG, 0, M, s, w);
    out[2 * k] = s;  // ws is only 4-B aligned: no 8-B store
    out[2 * k + 1] = w;
  }
}

template <int SEG, bool BATCHED = false, bool GROUPED = false>
__global__ __launch_bounds__(256) void segsum_ragged_t_kernel(
    int M, int K, int lda, int sstr, const float* __restrict__ A,
    float* __restrict__ S, long long strideA, long long strideS,
    GroupTable gt) {
  if constexpr (GROUPED) {
    for (int e = blockIdx.z; e < gt.groups; e += gridDim.z) {
      const GroupedEntry& d = gt.entry[e];
      if (!grouped_has_sums(d) ||
          (int)blockIdx.x >= (d.M + SEG - 1) / SEG)
        continue;
      segsum_ragged_t_band<SEG>(d.M, d.K, d.lda, d.sstr, d.A, S + d.ws_off,
                                blockIdx.x);
    }
    return;
  }
  if constexpr (BATCHED) {
    const long long z = blockIdx.z;
    A += z * strideA;
    S += z * strideS;
  }
  segsum_ragged_t_band<SEG>(M, K, lda, sstr, A, S, blockIdx.x);
}

// The ragged kernel.  Work decomposition, panel body, injector, verify and
// the per-element epilogue expression are sgemm_mfma's; what differs is the
// staging (fast 16-B path on a block and panel where it is legal, guarded
// 4-B path elsewhere — both give the same LDS contents, so C does not depend
// on which ran), the strip of a wave whose whole band lies below row M
// (zeros), and the guarded epilogue.
//
// TA / TB: that operand is transposed (lda / ldb then run along k).  Its fast
// path keeps panel it+1 in registers across panel it's MFMA loop: the loads
// are issued before the loop and the LDS writes after it, into buffer q^1,
// which was last read in panel it-1 and is protected by that panel's closing
// barrier; the barrier that closes panel it publishes it.  No barrier is
// added.
//
// BATCHED: one product per blockIdx.z; the prologue moves the pointers and the
// fault log to the entry and settles the entry's fast bits (header comment).
//
// GROUPED: one tile of some entry per blockIdx.x; the prologue looks the entry
// up in gt and replaces the sizes, leading dimensions, pointers, window
// stride, sstr and fast bits by the entry's own (header comment).  verify
// and inject stride are one value per entry, as the launchers pass them.
template <int BM, int BN, int BK, int WM, int WN, int MM, bool ABFT,
          bool INJECT, int OCC = 2, bool LOG = false, bool TA = false,
          bool TB = false, bool BATCHED = false, bool GROUPED = false>
__global__ __launch_bounds__(
    (tile_geom<BM, BN, BK, WM, WN, MM, ABFT>::THREADS),
    OCC) void sgemm_mfma_ragged(int M, int N, int K, int lda, int ldb, int ldc,
                                int fast, const float* __restrict__ A,
                                const float* __restrict__ B,
                                float* __restrict__ C, float alpha, float beta,
                                int verify_iters, int inject_stride, float tau,
                                float inj_mag, const float* __restrict__ SA,
                                int sstr, FaultLog flog, BatchStrides bs,
                                GroupTable gt) {
  using G = tile_geom<BM, BN, BK, WM, WN, MM, ABFT>;
  int bx = blockIdx.x, by = blockIdx.y;
  if constexpr (GROUPED) {
    const int e = grouped_entry_of(gt, blockIdx.x);
    const GroupedEntry& d = gt.entry[e];
    const int t = blockIdx.x - uniform(gt.tile_start[e]);
    const int tiles_x = uniform(d.tiles_x);
    by = t / tiles_x;
    bx = t - by * tiles_x;
    M = uniform(d.M), N = uniform(d.N), K = uniform(d.K);
    lda = uniform(d.lda), ldb = uniform(d.ldb), ldc = uniform(d.ldc);
    A = uniform(d.A), B = uniform(d.B), C = uniform(d.C);
    fast = ragged_fast_entry(uniform(d.fast), A, B, C);
    verify_iters = inject_stride = uniform(d.wstride);
    if constexpr (ABFT) {
      sstr = uniform(d.sstr);
      SA += uniform(d.ws_off);
    }
    if constexpr (LOG) {
      flog.counters += (long long)e * FLOG_N_COUNTERS;
      flog.events += (long long)e * flog.capacity * FLOG_EVENT_DWORDS;
    }
  }
  if constexpr (BATCHED) {
    const long long z = blockIdx.z;
    A += z * bs.A;
    B += z * bs.B;
    C += z * bs.C;
    fast = ragged_fast_entry(fast, A, B, C);
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

  using StA = stage_operand_t<BM, BK, THREADS>;
  using StB = stage_operand_t<BN, BK, THREADS>;
  typename StA::regs ra;  // a transposed operand's next panel (fast path)
  typename StB::regs rb;

  // Both operands transposed: A's registers are written to LDS half way
  // through the MFMA loop and B's are loaded only then, so that the two sets
  // are never live together (with both held across the loop the fused huge
  // kernels spill, docs/ABLATION.md section 16).
  constexpr bool SPLIT = TA && TB;

  // Starts the staging of panel k0 into buffer q.  A transposed operand on
  // its fast path is only loaded into ra / rb: the caller writes it to LDS
  // with stage_mid / stage_finish once buffer q may be overwritten.
  auto load_b_t = [&](int k0) __attribute__((always_inline)) {
    if (b_fast && k0 + BK <= K) StB::load(rb, B, ldb, jn0, k0, tid);
  };
  auto store_a_t = [&](int q, int k0) __attribute__((always_inline)) {
    if (a_fast && k0 + BK <= K) StA::store(ra, &lds[q * BUF], tid);
  };
  auto stage = [&](int q, int k0) __attribute__((always_inline)) {
    const bool k_full = k0 + BK <= K;
    if constexpr (TA) {
      if (a_fast && k_full)
        StA::load(ra, A, lda, im0, k0, tid);
      else
        stage_operand_guarded_t<BM, BK, THREADS>(&lds[q * BUF], A, lda, M, K,
                                                 im0, k0, tid, wave);
    } else {
      if (a_fast && k_full)
        stage_operand<BM, BK, THREADS>(&lds[q * BUF], A, lda, im0, k0, tid,
                                       wave);
      else
        stage_operand_guarded<BM, BK, THREADS>(&lds[q * BUF], A, lda, M, K,
                                               im0, k0, tid, wave);
    }
    if constexpr (TB) {
      if constexpr (!SPLIT) load_b_t(k0);
      if (!(b_fast && k_full))
        stage_operand_guarded_t<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B,
                                                 ldb, N, K, jn0, k0, tid,
                                                 wave);
    } else {
      if (b_fast && k_full)
        stage_operand<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B, ldb, jn0,
                                       k0, tid, wave);
      else
        stage_operand_guarded<BN, BK, THREADS>(&lds[q * BUF + BM * BK], B, ldb,
                                               N, K, jn0, k0, tid, wave);
    }
  };
  auto stage_mid = [&](int q, int k0) __attribute__((always_inline)) {
    if constexpr (SPLIT) {
      store_a_t(q, k0);
      load_b_t(k0);
    }
  };
  auto stage_finish = [&](int q, int k0) __attribute__((always_inline)) {
    if constexpr (TA || TB) {
      if constexpr (TA && !SPLIT) store_a_t(q, k0);
      if constexpr (TB) {
        if (b_fast && k0 + BK <= K)
          StB::store(rb, &lds[q * BUF + BM * BK], tid);
      }
      FT_PARA_SYNC();
    }
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
  stage_mid(0, 0);
  stage_finish(0, 0);
  if constexpr (ABFT) {
    // window 0 (panels 0..PPS-1); a grouped entry with K == 0 has no sums
    if (!GROUPED || K > 0) stage_strip(0, 0);
  }
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
        if constexpr (SPLIT) {
          if (kk == NKK / 2 && it + 1 < niter)
            stage_mid(q ^ 1, (it + 1) * BK);
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
      if (it + 1 < niter) stage_finish(q ^ 1, (it + 1) * BK);
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

// The RaggedFast bits of a launch, decided on the host.  BATCHED: from the
// leading dimensions alone; the kernel settles them per entry.
template <bool BATCHED = false>
int ragged_fast_bits(const GemmArgs& g, int lda, int ldb, int ldc) {
  const auto fast_ok = [](const void* p, int ld) {
    return (BATCHED || ((uintptr_t)p & 15) == 0) && ld % 4 == 0;
  };
  return (fast_ok(g.A, lda) ? RAGGED_FAST_A : 0) |
         (fast_ok(g.B, ldb) ? RAGGED_FAST_B : 0) |
         (fast_ok(g.C, ldc) ? RAGGED_FAST_C : 0);
}

// The encode of a fused ragged launch (nothing when !g.abft): the segment sums
// of A, one row per WM-row band, into g.ws (layout at
// sgemm_abft_workspace_floats).  BATCHED: one copy per entry, or one for all
// when A is shared; bs.SA becomes the distance between the copies.
template <int WM, bool TA, bool BATCHED = false>
void ragged_encode(const GemmArgs& g, int lda, Checksums& cs,
                   BatchStrides& bs) {
  if (!g.abft) return;
  const int M = g.M, K = g.K;
  cs.sstr = abft_sstr(K);
  cs.SA = g.ws;
  const int bands = (M + WM - 1) / WM;
  const int nA = BATCHED && g.strideA != 0 ? g.batch : 1;
  // one matrix's rows of the workspace (sgemm_abft_workspace_floats)
  const long long ws_each = 2LL * bands * cs.sstr;
  if constexpr (BATCHED) bs.SA = nA == 1 ? 0 : ws_each;
  RoctxRange rr(BATCHED ? "abft_encode_segsum_ragged_batched"
                        : "abft_encode_segsum_ragged");
  if constexpr (TA) {
    const int kblocks = (cs.sstr + 255) / 256;
    hipLaunchKernelGGL((segsum_ragged_t_kernel<WM, BATCHED>),
                       dim3(bands, kblocks < 1024 ? kblocks : 1024, nA),
                       dim3(256), 0, g.stream, M, K, lda, cs.sstr, g.A, g.ws,
                       g.strideA, ws_each, GroupTable{});
  } else {
    hipLaunchKernelGGL((segsum_ragged_kernel<WM, BATCHED>),
                       dim3(cs.sstr, nA), dim3(256), 0, g.stream, M, K, lda,
                       cs.sstr, g.A, g.ws, g.strideA, ws_each, GroupTable{});
  }
}

// Ragged launch of one tier: any M, N, K >= 1 on a ceil(M/BM) x ceil(N/BN)
// grid of sgemm_mfma_ragged.  g.lda / ldb / ldc of 0 mean packed (M, N, M; K
// for a transposed operand).  TA / TB must equal g.transA / g.transB:
// sgemm_tier_launch picks the translation unit that holds the combination.
// The workspace has one row per WM-row band of A, the last band partial.
// No allocation and no sync, so the launch can be captured.
//
// BATCHED (g.batch > 1, instantiated in the _ragged_batched translation units
// only): g.batch products on a ceil(M/BM) x ceil(N/BN) x batch grid, one
// encode launch and one GEMM launch.  strideA == 0 shares A: it is encoded
// once and every entry reads that workspace; otherwise g.ws holds g.batch
// copies of the single-launch layout.  The fast bits then come from the
// leading dimensions alone; the kernel settles them per entry.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false, bool BATCHED = false>
hipError_t launch_tier_ragged(const GemmArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  const int M = g.M, N = g.N, K = g.K;
  const int lda = g.lda ? g.lda : (TA ? K : M),
            ldb = g.ldb ? g.ldb : (TB ? K : N), ldc = g.ldc ? g.ldc : M;
  const int fast = ragged_fast_bits<BATCHED>(g, lda, ldb, ldc);
  const int bk_used = abft ? BKF : BK;
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN, BATCHED ? g.batch : 1);
  dim3 block(tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS);
  const int stride = window_stride((K + bk_used - 1) / bk_used,
                                   abft ? g.verify_windows : 1);
  BatchStrides bs;
  if constexpr (BATCHED) bs = {g.strideA, g.strideB, g.strideC, 0};
  Checksums cs;
  ragged_encode<WM, TA, BATCHED>(g, lda, cs, bs);
  RoctxRange rr_main(
      abft ? (inject ? (BATCHED ? "ft_sgemm_ragged_batched_abft_inject"
                                : "ft_sgemm_ragged_abft_inject")
                     : (BATCHED ? "ft_sgemm_ragged_batched_abft"
                                : "ft_sgemm_ragged_abft"))
           : (BATCHED ? "sgemm_ragged_batched_plain" : "sgemm_ragged_plain"));
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn = select_variant(
      abft, inject, flog.counters != nullptr,
      &sgemm_mfma_ragged<BM, BN, BK, WM, WN, MM, false, false, 2, false, TA,
                         TB, BATCHED>,
      [](auto inj, auto lg) {
        return &sgemm_mfma_ragged<BM, BN, BKF, WM, WN, MM, true,
                                  decltype(inj)::value, 2,
                                  decltype(lg)::value, TA, TB, BATCHED>;
      });
  hipLaunchKernelGGL(kfn, grid, block, 0, g.stream, M, N, K, lda, ldb, ldc,
                     fast, g.A, g.B, g.C, g.alpha, g.beta, stride, stride,
                     g.tau, g.inj_mag, cs.SA, cs.sstr, flog, bs, GroupTable{});
  return hipGetLastError();
}

// Grouped launch of one tier (instantiated in the _ragged_grouped translation
// units only): every entry of g.problems on a one-dimensional grid of
// sum_e ceil(M_e/BM) * ceil(N_e/BN) blocks, one encode launch (fused) and one
// GEMM launch, both reading the device table g.table that
// grouped_table_build filled for the same tier and arguments.  The scalar
// kernel arguments a table entry replaces are passed as zeros.  Checks
// nothing (sgemm_grouped_launch does); no allocation, no copy and no sync.
template <int BM, int BN, int BK, int BKF, int WM, int WN, int MM,
          bool TA = false, bool TB = false>
hipError_t launch_tier_ragged_grouped(const GroupedArgs& g) {
  const bool abft = g.abft, inject = g.inject;
  long long tiles = 0;
  int max_sstr = 0, max_bands = 0;
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    tiles += (long long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    if (p.M > 0 && p.N > 0 && p.K > 0) {
      const int sstr = abft_sstr(p.K), bands = (p.M + WM - 1) / WM;
      if (sstr > max_sstr) max_sstr = sstr;
      if (bands > max_bands) max_bands = bands;
    }
  }
  if (tiles == 0) return hipSuccess;  // every entry is empty
  const GroupTable gt = grouped_table_view(g.table, g.groups);
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
  RoctxRange rr_main(abft ? (inject ? "ft_sgemm_ragged_grouped_abft_inject"
                                    : "ft_sgemm_ragged_grouped_abft")
                          : "sgemm_ragged_grouped_plain");
  const FaultLog flog = attached_log(abft, g.log);
  const auto kfn = select_variant(
      abft, inject, flog.counters != nullptr,
      &sgemm_mfma_ragged<BM, BN, BK, WM, WN, MM, false, false, 2, false, TA,
                         TB, false, true>,
      [](auto inj, auto lg) {
        return &sgemm_mfma_ragged<BM, BN, BKF, WM, WN, MM, true,
                                  decltype(inj)::value, 2,
                                  decltype(lg)::value, TA, TB, false, true>;
      });
  dim3 block(tile_geom<BM, BN, BK, WM, WN, MM, false>::THREADS);
  hipLaunchKernelGGL(kfn, dim3((unsigned)tiles), block, 0, g.stream, 0, 0, 0,
                     0, 0, 0, 0, (const float*)nullptr, (const float*)nullptr,
                     (float*)nullptr, g.alpha, g.beta, 1, 1, g.tau, g.inj_mag,
                     (const float*)g.ws, 0, flog, BatchStrides{}, gt);
  return hipGetLastError();
}

}  // namespace ftsgemm
