// dispatch.hip — host-side launch layer for the CDNA4 SGEMM kernel family.
// Reference-parity role: the if/else kernel dispatch of
// /root/reference/kernel/ft_sgemm/sgemm.cu:110-199, driven by the generated
// tier table; each tier's kernels live in their own translation unit
// (csrc/generated/kernel_<tier>.hip).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ft_core.h"
#include "generated/tile_params.h"

namespace ftsgemm {

#define FT_DECL(name, BM, BN, BK, WM, WN, MM)              \
  hipError_t launch_tier_##name(const GemmArgs& g);         \
  hipError_t launch_tier_batched_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_##name(const GemmArgs& g);    \
  hipError_t launch_tier_ragged_tn_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_nt_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_tt_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_batched_##name(const GemmArgs& g);    \
  hipError_t launch_tier_ragged_batched_tn_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_batched_nt_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_batched_tt_##name(const GemmArgs& g);
FT_TIER_LIST(FT_DECL)
#undef FT_DECL

namespace {

// One row per tier, in FT_TIER_LIST order: the generator numbers
// FT_TIER_ID_<name> by position in that list, so a tier id indexes the table.
struct TierRow {
  hipError_t (*launch)(const GemmArgs&);
  hipError_t (*launch_batched)(const GemmArgs&);  // batch > 1
  // g.ragged, indexed by transA + 2 * transB: one translation unit each
  hipError_t (*launch_ragged[4])(const GemmArgs&);
  hipError_t (*launch_ragged_batched[4])(const GemmArgs&);  // and batch > 1
  int bm, bn, bk, wm;
};
const TierRow kTiers[FT_N_TIERS] = {
#define FT_ROW(name, BM, BN, BK, WM, WN, MM)                        \
  {launch_tier_##name,                                              \
   launch_tier_batched_##name,                                      \
   {launch_tier_ragged_##name, launch_tier_ragged_tn_##name,        \
    launch_tier_ragged_nt_##name, launch_tier_ragged_tt_##name},    \
   {launch_tier_ragged_batched_##name,                              \
    launch_tier_ragged_batched_tn_##name,                           \
    launch_tier_ragged_batched_nt_##name,                           \
    launch_tier_ragged_batched_tt_##name},                          \
   BM, BN, BK, WM},
    FT_TIER_LIST(FT_ROW)
#undef FT_ROW
};

const TierRow* tier_row(int tier) {
  return tier >= 0 && tier < FT_N_TIERS ? &kTiers[tier] : nullptr;
}

}  // namespace

// K is tested against the plain kernel's panel depth: every tier's fused
// depth bkf divides its bk (kernel_table.py), so the fused twin's whole
// panels follow.  M, N % 4: the f32x4 epilogue.
bool sgemm_tier_supported(int tier, int M, int N, int K) {
  const TierRow* t = tier_row(tier);
  return t && !(M % t->bm || N % t->bn || K % t->bk || M % 4 || N % 4);
}

// Every rule a launcher relies on; the launch_tier* templates check nothing
// themselves and are reachable only through sgemm_tier_launch.  (Stream-K's
// hipErrorNotSupported gates are a choice between two legal launches, not a
// rule, and stay in its launcher.)
const char* gemm_args_error(int tier, const GemmArgs& g) {
  constexpr int kMaxGridYZ = 65535;  // gridDim.y and .z
  const TierRow* t = tier_row(tier);
  if (!t) return "unknown tier id";
  if (g.M < 1 || g.N < 1 || g.K < 1) return "M, N and K must be >= 1";
  if (g.abft && !g.ws) return "a fused-ABFT launch needs its workspace ws";
  const uintptr_t ptrs =
      (uintptr_t)g.A | (uintptr_t)g.B | (uintptr_t)g.C | (uintptr_t)g.ws;
  if ((g.transA || g.transB) && !g.ragged)
    return "transA / transB need a ragged launch";
  if (g.ragged) {
    if (g.batch < 1 || g.batch > kMaxGridYZ) return "batch outside 1..65535";
    // a leading dimension may pad its rows, never cut them; a transposed
    // operand's rows run along k
    if ((g.lda && g.lda < (g.transA ? g.K : g.M)) ||
        (g.ldb && g.ldb < (g.transB ? g.K : g.N)) || (g.ldc && g.ldc < g.M))
      return "a leading dimension is shorter than its rows";
    if (ptrs & 3) return "A, B, C and ws must be 4-byte aligned";
    if ((g.N + t->bn - 1) / t->bn > kMaxGridYZ)
      return "N needs more than 65535 tile columns";
    if (g.batch > 1) {
      // blockIdx.z carries the entry.  Any stride: the kernel settles the
      // 16-B paths per entry (ft_ragged.hpp), so 4-B alignment is enough.
      if (g.strideA < 0 || g.strideB < 0)
        return "batch strides of A and B must be >= 0";
      // C entries are written: disjoint, or interleaved within a row of ldc
      // (heads inside a (tokens, heads*dim) tensor)
      const long long ldc = g.ldc ? g.ldc : g.M;
      const bool disjoint = g.strideC >= (g.N - 1) * ldc + g.M;
      const bool interleaved =
          g.strideC >= g.M && (g.batch - 1) * g.strideC + g.M <= ldc;
      if (!disjoint && !interleaved)
        return "C entries overlap (strideC >= (N-1)*ldc + M, or strideC >= M "
               "and (batch-1)*strideC + M <= ldc)";
    }
    return nullptr;
  }
  if (!sgemm_tier_supported(tier, g.M, g.N, g.K))
    return "the tier requires M,N,K multiples of its tile (M,N of 4 as well)";
  if (g.batch < 1 || g.batch > kMaxGridYZ) return "batch outside 1..65535";
  if (g.batch > 1) {
    // blockIdx.z carries the entry; 16-B staging and the f32x4 epilogue need
    // every entry's base 16-B aligned
    if (g.strideA < 0 || g.strideB < 0 || g.strideA % 4 || g.strideB % 4 ||
        g.strideC % 4)
      return "batch strides must be multiples of 4 floats, A's and B's >= 0";
    if (g.strideC < (long long)g.M * g.N)
      return "C entries must not overlap (strideC >= M*N)";
    if (ptrs & 15) return "A, B, C and ws must be 16-byte aligned";
  }
  return nullptr;
}

hipError_t sgemm_tier_launch(int tier, const GemmArgs& g) {
  if (gemm_args_error(tier, g)) return hipErrorInvalidValue;
  const TierRow& t = kTiers[tier];
  if (g.ragged) {
    const int tr = (g.transA ? 1 : 0) + (g.transB ? 2 : 0);
    return g.batch > 1 ? t.launch_ragged_batched[tr](g) : t.launch_ragged[tr](g);
  }
  return g.batch > 1 ? t.launch_batched(g) : t.launch(g);
}

size_t sgemm_abft_workspace_floats(int tier, const GemmArgs& g) {
  const TierRow* t = tier_row(tier);
  if (!t || g.M < 1 || g.N < 1 || g.K < 1) return 0;
  const size_t nA = g.batch > 1 && g.strideA != 0 ? g.batch : 1;
  return nA * 2 * (size_t)((g.M + t->wm - 1) / t->wm) * abft_sstr(g.K);
}

}  // namespace ftsgemm
