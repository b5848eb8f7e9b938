// ft_core.h — shared host API between the torch extension and the ft_sgemm
// CLI binary.
#pragma once

#include <hip/hip_runtime.h>

#include "fault_log.h"

namespace ftsgemm {

// Launch one of the six hand-tiled MFMA SGEMM kernels (tier id per
// generated/tile_params.h; abft selects the fused-ABFT twin, inject the
// always-on fault injector).  C = alpha*A*B^T + beta*C, column-major.
// When abft, `ws` must point to a device scratch buffer of
// sgemm_abft_workspace_floats(tier, M, N, K) fp32 elements (the launcher
// fills it with the segment checksums of A and B before the fused kernel).
// `log` (optional, fused variants only) attaches a caller-owned fault log
// (fault_log.h): the kernels' locate/correct path adds to its counters and
// appends one event per detected fault.  The launch neither zeroes,
// allocates nor syncs for it — counts accumulate until the caller clears
// them — and with log == nullptr the kernels write nothing.
hipError_t sgemm_tier_launch(int tier, bool abft, bool inject, int M, int N,
                             int K, const float* A, const float* B, float* C,
                             float alpha, float beta, float tau,
                             float inj_mag, int verify_windows, float* ws,
                             hipStream_t stream,
                             const FaultLog* log = nullptr);

bool sgemm_tier_supported(int tier, int M, int N, int K);

size_t sgemm_abft_workspace_floats(int tier, int M, int N, int K);

// Device self-test of the fused kernels' shared locate/correct
// (locate_selftest.hip): one single-wave block per case plants up to two
// accumulator faults in a synthetic FM x FN fragment tile of MM-wide MFMA
// fragments and corrects it with both the shipped function and the
// sweep-everything reference form.  idesc: 9 ints per case {nfault,
// (fm, fn, reg, lane) x 2}; fdesc: 3 floats per case {mag0, mag1, tau};
// out: [3][ncases][FM*FN*NREG][64] floats = {shipped, reference, clean}.
// All pointers are device pointers; (fm, fn, mm) must be a tier's shape.
hipError_t locate_selftest_launch(int fm, int fn, int mm, int ncases,
                                  const int* idesc, const float* fdesc,
                                  float amp, float* out, hipStream_t stream);

// Report variant of the self-test: runs only the shipped locate_correct, in
// its fault-log form, on the same descriptors.  Every case has a log of its
// own: counters is [ncases][FLOG_N_COUNTERS] and events
// [ncases][capacity][FLOG_EVENT_DWORDS] int32, both zeroed by the caller;
// the wave tile sits at origin (0, 0) with k range [0, 0).
// out: [ncases][FM*FN*NREG][64] floats, the corrected tile.
hipError_t locate_selftest_report_launch(int fm, int fn, int mm, int ncases,
                                         const int* idesc, const float* fdesc,
                                         float amp, float* out, int* counters,
                                         int* events, int capacity,
                                         hipStream_t stream);

// Detect variant of the self-test: runs only the fused kernels' shared
// detect and the locate's fp32 screen on the same descriptors, and returns
// what they computed.  out: [ncases][FM*FN*NREG + 1 + 2*FN][64] floats, lane
// fastest: the faulty tile, the wave residual, per fn the lane's partial
// sum p[fn], per fn 1.0 / 0.0 for a screen that passed / did not.
hipError_t detect_selftest_launch(int fm, int fn, int mm, int ncases,
                                  const int* idesc, const float* fdesc,
                                  float amp, float* out, hipStream_t stream);

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

// Non-fused ABFT baseline: per 256-wide K panel, rocBLAS
// sgemm + 6x sgemv + 2x saxpy + 2x sdot (call-chain parity with
// baseline_ft_sgemm.cuh:3-32).  Returns 0 on success; verdicts (squared
// residual norms) written to res_row/res_col (host pointers).
int baseline_ft_sgemm(int M, int N, int K, const float* A, const float* B,
                      float* C, float alpha, float beta,
                      const BaselineWorkspace& ws, int panel_k,
                      float* res_row, float* res_col, hipStream_t stream);

}  // namespace ftsgemm
