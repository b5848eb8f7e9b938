// ft_core.h — shared host API between the torch extension and the ft_sgemm
// CLI binary.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "fault_log.h"
#include "grouped_table.h"

namespace ftsgemm {

// One launch of the hand-tiled MFMA SGEMM kernels, host side only (never a
// kernel argument): C = alpha*A*B^T + beta*C, column-major.  abft selects
// the fused-ABFT twin, inject the always-on fault injector.
// When abft, `ws` must point to a device scratch buffer of
// sgemm_abft_workspace_floats(tier, g) fp32 elements (the launcher fills it
// with the segment checksums of A before the fused kernel).
// `log` (optional, fused variants only) attaches a caller-owned fault log
// (fault_log.h): the kernels' locate/correct path adds to its counters and
// appends one event per detected fault.  The launch neither zeroes,
// allocates nor syncs for it — counts accumulate until the caller clears
// them — and with log == nullptr the kernels write nothing.
//
// batch > 1 is a strided batch: for b in [0, batch), C_b = alpha * A_b *
// B_b^T + beta * C_b with X_b = X + b * strideX, strides in floats.  strideA
// and strideB may be 0 (one operand shared by every entry; a shared A is
// encoded once, so ws then holds one matrix's checksums, not batch of them).
// `log` points at the first of `batch` logs laid out as
// counters[batch][FLOG_N_COUNTERS] and
// events[batch][capacity][FLOG_EVENT_DWORDS]: entry b reports into log b.
// A batched launch always takes the classic tile-per-workgroup path
// (FT_SGEMM_STREAMK has no effect on it); batch == 1 is the single launch and
// ignores the strides.
//
// ragged lifts the tile fit: any M, N, K >= 1, leading dimensions lda / ldb
// / ldc (0 = packed), base pointers with only fp32 alignment.  The ragged
// twin of the classic kernel runs (ft_ragged.hpp) on ceil tile counts.  A
// fault injected into an edge tile's padding is logged with its padded
// coordinates (fault_log.h).  ragged with batch > 1 is a strided batch of
// such products in one launch: any strides (A's and B's >= 0, 0 = shared),
// no alignment beyond fp32 for any entry, workspace and logs laid out as for
// the tiled batch.  C's entries may be disjoint or interleaved within a row
// of ldc (entry b's rows inside the rows of one wider matrix), never
// overlapping.  ragged with batch == 1 is the single ragged launch.
//
// transA / transB (ragged launches only) take that operand transposed, i.e.
// row-major: with transA, element (i, k) of the logical M x K matrix A is at
// A[k + i*lda] with lda >= K (0 = packed = K); transB likewise for B with
// ldb >= K.  C, the workspace and its size are unchanged, and the result has
// the bits of the untransposed launch on the transposed copy.
//
// sk_grid > 0 (single ragged launches on a tier with a stream-K twin only)
// runs the ragged stream-K decomposition (ft_ragged_streamk.hpp) on sk_grid
// workgroups instead of one workgroup per tile: the work is the list of
// ceil(M/BM) * ceil(N/BN) * ceil(K/64) units (one 64-k window of one tile),
// cut into sk_grid balanced contiguous ranges; a grid beyond the unit count is
// clamped to it.  sk_partials is the caller's buffer of
// sgemm_streamk_partials_floats(tier, sk_grid) floats, 16-byte aligned, that
// the split tiles are combined through; nothing in it has to be initialised
// and nothing is kept in it between launches.  The launch allocates nothing,
// does not sync and reads no environment variable, so it can be captured.
// sk_grid == 0 is the classic ragged launch.
//
// Which shapes, strides, leading dimensions and alignments each of the
// forms accepts is stated once, in gemm_args_error.
struct GemmArgs {
  bool abft, inject;
  int M, N, K;
  const float *A, *B;
  float* C;
  float alpha, beta, tau, inj_mag;
  int verify_windows;  // <= 0: the default of 20
  float* ws = nullptr;
  hipStream_t stream = 0;
  const FaultLog* log = nullptr;
  int batch = 1;
  long long strideA = 0, strideB = 0, strideC = 0;
  bool ragged = false;
  int lda = 0, ldb = 0, ldc = 0;  // ragged only; 0 = packed
  bool transA = false, transB = false;  // ragged only
  int sk_grid = 0;                // ragged stream-K workgroups; 0 = classic
  float* sk_partials = nullptr;   // caller-owned, sk_grid > 0 only
};

// The launch rules: nullptr when sgemm_tier_launch(tier, g) may launch g,
// otherwise a static message naming the rule g breaks (tier id per
// generated/tile_params.h).
const char* gemm_args_error(int tier, const GemmArgs& g);

// Launch tier `tier`; hipErrorInvalidValue, with nothing launched, when
// gemm_args_error(tier, g) has a message.
hipError_t sgemm_tier_launch(int tier, const GemmArgs& g);

// The tile fit of a tiled (non-ragged) launch alone.
bool sgemm_tier_supported(int tier, int M, int N, int K);

// Row stride of the ABFT workspace: round_up(K, 64), so the fused kernel's
// 64-k strip loads never cross rows.
inline int abft_sstr(int K) { return (K + 63) & ~63; }

// Floats of g.ws a fused launch of g needs (g.ws itself is not looked at; 0
// for an unknown tier or an empty shape).  Layout: one row per WM-row band of
// A, ceil(M / WM) of them (a tiled M is a multiple of WM), each of
// 2 * abft_sstr(K) floats holding the (plain, row-weighted) segment-sum
// pairs INTERLEAVED at [2k], [2k+1]; a batch whose entries have their own A
// (batch > 1, strideA != 0) holds `batch` consecutive copies.  B-side sums
// are not needed by the ratio-locate scheme.
size_t sgemm_abft_workspace_floats(int tier, const GemmArgs& g);

// The device grid of a ragged stream-K launch of g on `tier` (g.sk_grid and
// g.sk_partials are not looked at): CU count x the occupancy of the kernel
// variant g selects, always the one without a fault log so that attaching a
// log cannot change the decomposition, clamped to the unit count.  0 for a
// tier without a stream-K twin or a g that is no single ragged launch.
// Launches nothing.
int sgemm_ragged_streamk_grid(int tier, const GemmArgs& g);

// Floats of GemmArgs::sk_partials a stream-K launch on `grid` workgroups
// needs: two BM x BN slots per workgroup (head and tail partial).  0 for a
// tier without a stream-K twin or grid < 1.
size_t sgemm_streamk_partials_floats(int tier, int grid);

// Inject+verify cadence: `steps` K-steps of a tile (classic: K / BK panels,
// stream-K: 64-k units) in ~`windows` windows of whole steps (reference: 20
// per GEMM, period K/20, ft_sgemm_huge.cuh:324-327).  Returns steps per
// window.  Here because the launchers (tier_launch.hpp) and the grouped
// table (dispatch.hip) must agree on it.
inline int window_stride(int steps, int windows) {
  const int stride = steps / (windows > 0 ? windows : 20);
  return stride < 1 ? 1 : stride;
}

// One product of a grouped launch, host side: GemmArgs' ragged fields for one
// entry.  lda / ldb / ldc of 0 mean packed, as there.
struct GroupedProblem {
  const float *A, *B;
  float* C;
  int M, N, K;
  int lda, ldb, ldc;
};

// One grouped launch of the ragged kernels: `groups` products, entry e being
// C_e = alpha * A_e * B_e^T + beta * C_e with its own sizes, leading
// dimensions and pointers (problems[e], a host array), in one launch on a
// one-dimensional grid over the tiles of all entries.  alpha, beta, tau,
// inj_mag, verify_windows and the transpose flags are common to the launch.
// There is no limit on groups; the tiles of all entries together must not
// exceed 2^31 - 1.
//
// Unlike a single ragged launch an entry may be empty.  M_e == 0 or N_e == 0:
// no tiles, no workspace, its log untouched.  K_e == 0 with M_e, N_e > 0:
// C_e = beta * C_e (exact zeros, C never read, for beta == 0); such an entry
// reads no operand and no workspace and injects nothing.
//
// `table` is device memory of grouped_table_bytes(groups) bytes holding what
// grouped_table_build wrote for this tier and these arguments (abft,
// verify_windows, the transpose flags and problems all enter it): the kernels
// read the entries from it, the launch reads problems only to validate and to
// size the grids.  `ws` (fused) holds sgemm_grouped_workspace_floats floats;
// every entry's A is encoded by itself into its own region.  `log` points at
// the first of `groups` logs laid out like a batch's (GemmArgs): entry e
// reports into log e.
//
// sk_grid > 0 (tiers with a stream-K twin only) runs the grouped stream-K
// decomposition (ft_ragged_grouped_streamk.hpp) on sk_grid workgroups: the
// work is the list of units of all entries, entry e having
// tiles_e * max(1, ceil(K_e / 64)) of them, ordered by entry, tile (bx
// fastest) and k, cut into sk_grid balanced contiguous ranges; a grid beyond
// the unit count is clamped to it.  A K_e == 0 entry has one empty unit per
// tile, whose owner writes beta * C_e.  `table` is then
// grouped_streamk_table_bytes(groups) bytes, built with the same sk_grid > 0,
// and sk_partials the caller's buffer of
// sgemm_streamk_partials_floats(tier, sk_grid) floats, 16-byte aligned.
// Entry e's fully-owned tiles have the bits of the classic grouped launch;
// split tiles are summed in a fixed order, so every run gives the same bits.
// sk_grid == 0 is the classic grouped launch.
struct GroupedArgs {
  bool abft, inject;
  float alpha, beta, tau, inj_mag;
  int verify_windows;  // <= 0: the default of 20
  bool transA = false, transB = false;
  int groups = 0;
  const GroupedProblem* problems = nullptr;  // host, groups of them
  const void* table = nullptr;               // device
  float* ws = nullptr;
  hipStream_t stream = 0;
  const FaultLog* log = nullptr;
  int sk_grid = 0;               // grouped stream-K workgroups; 0 = classic
  float* sk_partials = nullptr;  // caller-owned, sk_grid > 0 only
};

// The rules of a grouped launch, stated once: nullptr when g's problems may
// be launched on `tier` (g.table and g.ws are not looked at), otherwise a
// static message naming the rule g breaks.  Per entry
// they are the single ragged launch's (gemm_args_error) with the empty cases
// above allowed.  The footprints [C_e, C_e + (N_e-1)*ldc_e + M_e) of the
// entries that write must be pairwise disjoint as address intervals: entries
// interleaved within a row of a wider matrix, which a strided batch accepts,
// are not supported in this form.
const char* grouped_args_error(int tier, const GroupedArgs& g);

// Fills host_table (grouped_table_bytes(g.groups) bytes of host memory,
// grouped_table.h) with the table of g on `tier`: tile-start prefix with the
// total last, and
// per entry the pointers, sizes, resolved leading dimensions, the fast bits
// the leading dimensions allow, the window stride
// window_stride(ceil(K_e / bk_used), verify_windows), sstr and the workspace
// offset.  With g.sk_grid > 0 host_table is
// grouped_streamk_table_bytes(g.groups) bytes and the stream-K section
// (unit-start prefix, per-entry verify stride in units) is filled behind
// the classic table, which is the same bytes either way.  g.table and g.ws
// are not looked at.  The caller copies the table
// to the device.  Returns grouped_args_error's message, nothing written, when
// there is one.
const char* grouped_table_build(int tier, const GroupedArgs& g,
                                void* host_table);

// Floats of g.ws a fused grouped launch needs: sum_e 2 * ceil(M_e / WM) *
// abft_sstr(K_e) over the entries with M_e, N_e, K_e > 0, entry e's region
// laid out like a single launch's (sgemm_abft_workspace_floats) and starting
// where entry e-1's ends.
size_t sgemm_grouped_workspace_floats(int tier, const GroupedArgs& g);

// Launch g on tier `tier`: one encode launch (fused) and one GEMM launch.
// hipErrorInvalidValue, with nothing launched, when grouped_args_error has a
// message, g.table is missing or a fused launch that needs one has no g.ws.  No allocation, no copy and no sync, so it can be captured.
// g.sk_grid > 0: the encode, the grouped stream-K kernel and the fixup pass.
hipError_t sgemm_grouped_launch(int tier, const GroupedArgs& g);

// The device grid of a grouped stream-K launch of g on `tier` (g.sk_grid,
// g.sk_partials and g.table are not looked at): CU count x the occupancy of
// the kernel variant g selects, always the one without a fault log, clamped
// to the unit count.  0 for a tier without a stream-K twin, a g that breaks a
// rule or one without units.  Launches nothing.
int sgemm_grouped_streamk_grid(int tier, const GroupedArgs& g);

// Work units of a grouped stream-K launch of g on `tier`: sum over the
// entries of ceil(M_e/BM) * ceil(N_e/BN) * max(1, ceil(K_e/64)).  A launch
// runs on min(sk_grid, units) workgroups and needs
// sgemm_streamk_partials_floats(tier, that) floats of partials.  0 for an
// unknown tier or sizes outside grouped_args_error's range.
long long sgemm_grouped_streamk_units(int tier, const GroupedArgs& g);

// Device self-test of the fused kernels' shared detect / locate / correct
// (locate_selftest.hip): one single-wave block per case plants up to two
// accumulator faults in a synthetic FM x FN fragment tile of MM-wide MFMA
// fragments, NREG accumulators per lane each, and runs one of three modes
// on it.  All outputs are fp32, element e = (fm*FN + fn)*NREG + reg, lane
// fastest.
enum SelftestMode {
  // Corrects the tile with both the shipped locate_correct and the
  // sweep-everything reference form.
  // out: [3][ncases][FM*FN*NREG][64] = {shipped, reference, clean}.
  SELFTEST_LOCATE,
  // Only the shipped locate_correct, in its fault-log form.  Every case has
  // a log of its own: counters is [ncases][FLOG_N_COUNTERS] and events
  // [ncases][capacity][FLOG_EVENT_DWORDS] int32, both zeroed by the caller;
  // the wave tile sits at origin (0, 0) with k range [0, 0).
  // out: [ncases][FM*FN*NREG][64], the corrected tile.
  SELFTEST_REPORT,
  // Only the shared detect and the locate's fp32 screen; nothing is
  // corrected.  out: [ncases][FM*FN*NREG + 1 + 2*FN][64]: the faulty tile as
  // the detect saw it, the wave residual (the same in every lane), per fn
  // the lane's partial sum p[fn], per fn 1.0 / 0.0 for a screen that passed
  // / did not (wave-uniform).
  SELFTEST_DETECT,
};

// idesc: 9 ints per case {nfault, (fm, fn, reg, lane) x 2}; fdesc: 3 floats
// per case {mag0, mag1, tau}; clean accumulators are a hash in (-amp, amp).
// All pointers are device pointers; (fm, fn, mm) must be a tier's shape.
// counters / events / capacity: SELFTEST_REPORT only.
struct SelftestArgs {
  int fm, fn, mm, ncases;
  const int* idesc;
  const float* fdesc;
  float amp;
  float* out;
  int* counters = nullptr;
  int* events = nullptr;
  int capacity = 0;
  hipStream_t stream = 0;
};

hipError_t selftest_launch(SelftestMode mode, const SelftestArgs& a);

// rocBLAS paths (kernel id 0 oracle and the id-10 non-fused ABFT baseline,
// reference: cuBLAS at sgemm.cu:108 / include/baseline_ft_sgemm.cuh).
// Implemented in rocblas_path.hip.
struct BaselineWorkspace {
  // device buffers, all fp32; caller owns allocation
  float* ones;     // max(M, N) ones
  float* row_c;    // M   (C row sums)
  float* col_c;    // N   (C column sums)
  float* s_a;      // panel_k (A-panel column sums)
  float* s_b;      // panel_k (B-panel row sums)
  float* ref_row;  // M   (maintained row checksum)
  float* ref_col;  // N   (maintained col checksum)
  float* d_res;    // 2 * ceil(K / panel_k)  (device-side dot verdict slot
                   // pair per verified panel, stream-ordered; the host
                   // reduces to the WORST panel's verdicts)
};

int rocblas_sgemm_nt(int M, int N, int K, const float* A, const float* B,
                     float* C, float alpha, float beta, hipStream_t stream);

// Test seam of the baseline chain: one fault put into the running C right
// after the GEMM of panel `panel`, before that panel's checksum update and
// verdict.  C[i + j*M] += value, or = value when overwrite.
struct BaselineFault {
  int panel, i, j;
  float value;
  bool overwrite;
};

// One verdict of the baseline chain: the squared residual norms computed
// after panel `panel`.
struct BaselineVerdict {
  int panel;
  float res_row, res_col;
};

// Non-fused ABFT baseline: per 256-wide K panel, rocBLAS
// sgemm + 6x sgemv + 2x saxpy + 2x sdot (call-chain parity with
// baseline_ft_sgemm.cuh:3-32).  Returns 0 on success; verdicts (squared
// residual norms) written to res_row/res_col (host pointers): the worst
// verified panel's, and NaN or Inf whenever any panel's was.
// fault (nullptr = none) is the seam above; a fault outside
// 0 <= panel < ceil(K / panel_k), 0 <= i < M, 0 <= j < N returns -2 before
// anything is launched.  verdicts (nullptr = not wanted) receives every
// verdict computed, in panel order.
int baseline_ft_sgemm(int M, int N, int K, const float* A, const float* B,
                      float* C, float alpha, float beta,
                      const BaselineWorkspace& ws, int panel_k,
                      float* res_row, float* res_col, hipStream_t stream,
                      const BaselineFault* fault,
                      std::vector<BaselineVerdict>* verdicts);

}  // namespace ftsgemm
