// cli_main.hip — the `ft_sgemm` CLI: verification pass + GFLOPS sweep.
//
// API-compatible re-implementation of the reference benchmark driver
// (/root/reference/kernel/ft_sgemm/sgemm.cu):
//   usage: ft_sgemm [START END STEP KSTART KEND]   (defaults 1024 6144 512 0 16)
// * verification pass: every kernel id in [KSTART, KEND] is checked against
//   rocBLAS (the reference checks against cuBLAS, sgemm.cu:100-229) with the
//   |diff|>1e-2 AND rel>1e-2 tolerance of utils.cu:61-77;
// * perf sweep: kernel ids {0,1..6,10,11..16} x sizes START..END step STEP,
//   5 timed reps each, alpha=1 beta=-1.5, GFLOPS = 2*M*N*K*5/t
//   (protocol parity: sgemm.cu:21,24,234,431-435).
// The FT kernels (ids 11-16) run with the always-on fault injector, so a
// passing verification proves in-kernel detect+locate+correct end to end
// (SURVEY.md section 4 item 2).  Set FT_SGEMM_NO_INJECT=1 to measure the
// ABFT overhead without injection.  Set FT_SGEMM_REPORT=1 to attach a fault
// log to every fused id in the verification pass and print its counters.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ft_core.h"

#define HIP_CALL(x)                                                       \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_),   \
              __FILE__, __LINE__);                                        \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

namespace {

const char* kNames[17] = {
    "cublas",          // id 0: vendor BLAS (rocBLAS on this hardware); name
                       // kept for table parity with README.md:38-53
    "kernel_sgemm_small", "kernel_sgemm_medium", "kernel_sgemm_large",
    "kernel_sgemm_tall",  "kernel_sgemm_wide",   "kernel_sgemm_huge",
    "kernel_7", "kernel_8", "kernel_9",
    "abft_baseline",
    "abft_kernel_small", "abft_kernel_medium", "abft_kernel_large",
    "abft_kernel_tall",  "abft_kernel_wide",   "abft_kernel_huge"};

constexpr float kTau = 9500.f, kInj = 10000.f;

// fused-ABFT segment-checksum scratch, grown on demand
float* abft_ws(size_t floats) {
  static float* buf = nullptr;
  static size_t cap = 0;
  if (floats > cap) {
    if (buf) (void)hipFree(buf);
    HIP_CALL(hipMalloc(&buf, floats * sizeof(float)));
    cap = floats;
  }
  return buf;
}

bool run_kernel(int kid, int M, int N, int K, const float* dA,
                const float* dB, float* dC, float alpha, float beta,
                const ftsgemm::BaselineWorkspace& ws, bool inject,
                const ftsgemm::FaultLog* log = nullptr) {
  ftsgemm::GemmArgs g{/*abft=*/false, /*inject=*/false, M, N, K, dA, dB, dC,
                      alpha, beta, kTau, kInj, /*verify_windows=*/20};
  if (kid >= 1 && kid <= 6)
    return ftsgemm::sgemm_tier_launch(kid - 1, g) == hipSuccess;
  if (kid >= 11 && kid <= 16) {
    g.abft = true;
    g.inject = inject;
    g.ws = abft_ws(ftsgemm::sgemm_abft_workspace_floats(kid - 11, g));
    g.log = log;
    return ftsgemm::sgemm_tier_launch(kid - 11, g) == hipSuccess;
  }
  if (kid == 10) {
    // panel width sized for MI355X (the reference's 256 is T4-sized: at
    // these GFLOPS the per-panel full-C gemv sweeps and launch overhead
    // dominate; FT_SGEMM_PANEL_K overrides)
    static const int panel_k = [] {
      const char* e = getenv("FT_SGEMM_PANEL_K");
      int p = e ? atoi(e) : 1024;
      // the verdict-slot buffer is sized for panel_k >= 64 (2*(maxn/64+2))
      return p < 64 ? 64 : p;
    }();
    float r0 = 0, r1 = 0;
    return ftsgemm::baseline_ft_sgemm(M, N, K, dA, dB, dC, alpha, beta, ws,
                                      panel_k, &r0, &r1, 0, /*fault=*/nullptr,
                                      /*verdicts=*/nullptr) == 0;
  }
  // ids 0, 7, 8, 9: rocBLAS (reference falls back to cuBLAS, sgemm.cu:197)
  return ftsgemm::rocblas_sgemm_nt(M, N, K, dA, dB, dC, alpha, beta, 0) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  int start = 1024, end = 6144, gap = 512, k0 = 0, k1 = 16;
  if (argc >= 6) {
    start = atoi(argv[1]);
    end = atoi(argv[2]);
    gap = atoi(argv[3]);
    k0 = atoi(argv[4]);
    k1 = atoi(argv[5]);
  }
  const char* no_inj = getenv("FT_SGEMM_NO_INJECT");
  const bool inject = !(no_inj && strcmp(no_inj, "0") != 0);
  const char* json_env = getenv("FT_SGEMM_JSON");  // machine-readable lines
  FILE* jf = nullptr;
  if (json_env && *json_env) jf = fopen(json_env, "w");
  // FT_SGEMM_REPORT: fault log for the fused ids of the verification pass
  const char* rep_env = getenv("FT_SGEMM_REPORT");
  const bool report = rep_env && *rep_env && strcmp(rep_env, "0") != 0;
  ftsgemm::FaultLog flog;
  if (report) {
    flog.capacity = 1024;
    HIP_CALL(hipMalloc(&flog.counters, ftsgemm::FLOG_N_COUNTERS * sizeof(int)));
    HIP_CALL(hipMalloc(&flog.events, (size_t)flog.capacity *
                                         ftsgemm::FLOG_EVENT_DWORDS *
                                         sizeof(int)));
  }
  const int reps = 5;
  const float alpha = 1.f;
  // END < START runs the verification pass only (tools/race_check.sh);
  // buffers must still cover the verify size
  const size_t maxn = (size_t)(end > start ? end : start);
  const size_t bytes = maxn * maxn * sizeof(float);

  // Host operands: uniform (-0.9, 0.9), deterministic seed (reference:
  // srand(10) + generate_random_matrix, sgemm.cu:12 / utils.cu:23).
  std::vector<float> hA(maxn * maxn), hB(maxn * maxn);
  {
    std::mt19937 rng(10);
    std::uniform_real_distribution<float> d(-0.9f, 0.9f);
    for (auto& v : hA) v = d(rng);
    for (auto& v : hB) v = d(rng);
  }

  float *dA, *dB, *dC, *dCref;
  HIP_CALL(hipMalloc(&dA, bytes));
  HIP_CALL(hipMalloc(&dB, bytes));
  HIP_CALL(hipMalloc(&dC, bytes));
  HIP_CALL(hipMalloc(&dCref, bytes));
  HIP_CALL(hipMemcpy(dA, hA.data(), bytes, hipMemcpyHostToDevice));
  HIP_CALL(hipMemcpy(dB, hB.data(), bytes, hipMemcpyHostToDevice));

  // Baseline (id 10) checksum workspace
  float *ws_ones, *ws_rowc, *ws_colc, *ws_sa, *ws_sb, *ws_rrow, *ws_rcol,
      *ws_dres;
  HIP_CALL(hipMalloc(&ws_ones, maxn * sizeof(float)));
  HIP_CALL(hipMalloc(&ws_rowc, maxn * sizeof(float)));
  HIP_CALL(hipMalloc(&ws_colc, maxn * sizeof(float)));
  HIP_CALL(hipMalloc(&ws_sa, maxn * sizeof(float)));  // >= panel_k
  HIP_CALL(hipMalloc(&ws_sb, maxn * sizeof(float)));
  HIP_CALL(hipMalloc(&ws_rrow, maxn * sizeof(float)));
  HIP_CALL(hipMalloc(&ws_rcol, maxn * sizeof(float)));
  // verdict slot pairs: one per verified panel (worst-panel semantics);
  // panel_k >= 64 always, so maxn/64 bounds the panel count
  HIP_CALL(hipMalloc(&ws_dres, 2 * (maxn / 64 + 2) * sizeof(float)));
  {
    std::vector<float> ones(maxn, 1.f);
    HIP_CALL(hipMemcpy(ws_ones, ones.data(), maxn * sizeof(float),
                       hipMemcpyHostToDevice));
  }
  ftsgemm::BaselineWorkspace ws{ws_ones, ws_rowc, ws_colc, ws_sa,
                                ws_sb,   ws_rrow, ws_rcol, ws_dres};

  // ---------------- verification pass ----------------
  const int vM = start, vN = start, vK = start;
  std::vector<float> hC(maxn * maxn), hCref(maxn * maxn);
  char fault_json[17][128] = {};  // per id: the verify pass's fault counts
  printf("verify at M=N=K=%d\n", vM);
  for (int kid = k0; kid <= k1 && kid <= 16; ++kid) {
    ftsgemm::rocblas_sgemm_nt(vM, vN, vK, dA, dB, dCref, 1.f, 0.f, 0);
    HIP_CALL(hipMemset(dC, 0, (size_t)vM * vN * sizeof(float)));
    const bool logged = report && kid >= 11 && kid <= 16;
    if (logged)
      HIP_CALL(hipMemset(flog.counters, 0,
                         ftsgemm::FLOG_N_COUNTERS * sizeof(int)));
    if (!run_kernel(kid, vM, vN, vK, dA, dB, dC, 1.f, 0.f, ws, inject,
                    logged ? &flog : nullptr)) {
      printf("kernel %2d %-20s LAUNCH FAILED\n", kid, kNames[kid]);
      continue;
    }
    HIP_CALL(hipGetLastError());
    HIP_CALL(hipDeviceSynchronize());
    HIP_CALL(hipMemcpy(hC.data(), dC, (size_t)vM * vN * sizeof(float),
                       hipMemcpyDeviceToHost));
    HIP_CALL(hipMemcpy(hCref.data(), dCref, (size_t)vM * vN * sizeof(float),
                       hipMemcpyDeviceToHost));
    // FT_SGEMM_DUMP=<dir>: write the raw verification output per kernel id
    // (bit-exact comparison between the normal and FT_PARANOID builds —
    // tools/race_check.sh)
    if (const char* dd = getenv("FT_SGEMM_DUMP")) {
      char path[512];
      snprintf(path, sizeof path, "%s/k%02d.bin", dd, kid);
      if (FILE* df = fopen(path, "wb")) {
        fwrite(hC.data(), sizeof(float), (size_t)vM * vN, df);
        fclose(df);
      }
    }
    bool ok = true;
    for (size_t i = 0; i < (size_t)vM * vN; ++i) {
      float diff = fabsf(hC[i] - hCref[i]);
      if (diff > 1e-2f && diff / fabsf(hCref[i]) > 1e-2f) {  // utils.cu:61-77
        printf("kernel %2d %-20s MISMATCH at %zu: %f vs %f\n", kid,
               kNames[kid], i, hC[i], hCref[i]);
        ok = false;
        break;
      }
    }
    if (ok) printf("kernel %2d %-20s verified\n", kid, kNames[kid]);
    if (logged) {
      int cnt[ftsgemm::FLOG_N_COUNTERS];
      HIP_CALL(hipMemcpy(cnt, flog.counters, sizeof cnt,
                         hipMemcpyDeviceToHost));
      printf("faults: tripped %d corrected %d uncorrected %d unlocated %d\n",
             cnt[ftsgemm::FLOG_TRIPPED], cnt[ftsgemm::FLOG_CORRECTED],
             cnt[ftsgemm::FLOG_UNCORRECTED], cnt[ftsgemm::FLOG_UNLOCATED]);
      // kept for this id's JSON lines (written by the sweep below)
      snprintf(fault_json[kid], sizeof fault_json[kid],
               ", \"tripped\": %d, \"corrected\": %d, \"uncorrected\": %d, "
               "\"unlocated\": %d",
               cnt[ftsgemm::FLOG_TRIPPED], cnt[ftsgemm::FLOG_CORRECTED],
               cnt[ftsgemm::FLOG_UNCORRECTED], cnt[ftsgemm::FLOG_UNLOCATED]);
    }
  }

  // ---------------- perf sweep ----------------
  const int sweep_ids[14] = {0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16};
  const float beta = -1.5f;  // sgemm.cu:234
  printf("\nMatrix Size");
  for (int n = start; n <= end; n += gap) printf("|%8d", n);
  printf("|\n");
  // FT_SGEMM_SWEEP_IDS="6,16": restrict the sweep to a comma-separated
  // kernel-id list (benchmarking/bisection aid; default = all 14 rows,
  // reference parity)
  bool row_on[17];
  for (int i = 0; i < 17; ++i) row_on[i] = true;
  if (const char* ids = getenv("FT_SGEMM_SWEEP_IDS")) {
    for (int i = 0; i < 17; ++i) row_on[i] = false;
    const char* p = ids;
    while (*p) {
      int v = atoi(p);
      if (v >= 0 && v <= 16) row_on[v] = true;
      while (*p && *p != ',') ++p;
      if (*p == ',') ++p;
    }
  }
  for (int idx = 0; idx < 14; ++idx) {
    const int kid = sweep_ids[idx];
    if (!row_on[kid]) continue;
    printf("%s", kNames[kid]);
    for (int n = start; n <= end; n += gap) {
      const int M = n, N = n, K = n;
      hipEvent_t beg, fin;
      HIP_CALL(hipEventCreate(&beg));
      HIP_CALL(hipEventCreate(&fin));
      // one warm-up launch (not in the reference; excluded from timing)
      run_kernel(kid, M, N, K, dA, dB, dC, alpha, beta, ws, inject);
      HIP_CALL(hipDeviceSynchronize());
      HIP_CALL(hipEventRecord(beg));
      for (int r = 0; r < reps; ++r) {
        run_kernel(kid, M, N, K, dA, dB, dC, alpha, beta, ws, inject);
        HIP_CALL(hipDeviceSynchronize());
      }
      HIP_CALL(hipEventRecord(fin));
      HIP_CALL(hipEventSynchronize(fin));
      float ms = 0;
      HIP_CALL(hipEventElapsedTime(&ms, beg, fin));
      double gflops = 2.0 * M * N * K * reps / (ms * 1e-3) / 1e9;
      printf("|%8.0f", gflops);
      if (jf)
        fprintf(jf,
                "{\"kernel_id\": %d, \"name\": \"%s\", \"n\": %d, "
                "\"gflops\": %.1f, \"reps\": %d, \"inject\": %s%s}\n",
                kid, kNames[kid], n, gflops, reps,
                (kid >= 11 && inject) ? "true" : "false", fault_json[kid]);
      HIP_CALL(hipEventDestroy(beg));
      HIP_CALL(hipEventDestroy(fin));
      fflush(stdout);
    }
    printf("|\n");
  }
  if (jf) fclose(jf);
  return 0;
}
