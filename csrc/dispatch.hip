// dispatch.hip — host-side launch layer for the CDNA4 SGEMM kernel family.
// Reference-parity role: the if/else kernel dispatch of
// /root/reference/kernel/ft_sgemm/sgemm.cu:110-199, driven by the generated
// tier table; each tier's kernels live in their own translation unit
// (csrc/generated/kernel_<tier>.hip).

#include <hip/hip_runtime.h>

#include "ft_core.h"
#include "generated/tile_params.h"

namespace ftsgemm {

#define FT_DECL(name, BM, BN, BK, WM, WN, MM)              \
  hipError_t launch_tier_##name(const GemmArgs& g);         \
  hipError_t launch_tier_batched_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_##name(const GemmArgs& g);  \
  size_t abft_ws_floats_##name(int M, int N, int K);        \
  size_t abft_ws_floats_ragged_##name(int M, int N, int K);
FT_TIER_LIST(FT_DECL)
#undef FT_DECL

namespace {

// One row per tier, in FT_TIER_LIST order: the generator numbers
// FT_TIER_ID_<name> by position in that list, so a tier id indexes the table.
struct TierRow {
  hipError_t (*launch)(const GemmArgs&);
  hipError_t (*launch_batched)(const GemmArgs&);  // batch > 1
  hipError_t (*launch_ragged)(const GemmArgs&);   // g.ragged
  size_t (*ws_floats)(int, int, int);
  size_t (*ws_floats_ragged)(int, int, int);
  int bm, bn, bk;
};
const TierRow kTiers[FT_N_TIERS] = {
#define FT_ROW(name, BM, BN, BK, WM, WN, MM)                   \
  {launch_tier_##name,    launch_tier_batched_##name,           \
   launch_tier_ragged_##name, abft_ws_floats_##name,            \
   abft_ws_floats_ragged_##name, BM, BN, BK},
    FT_TIER_LIST(FT_ROW)
#undef FT_ROW
};

const TierRow* tier_row(int tier) {
  return tier >= 0 && tier < FT_N_TIERS ? &kTiers[tier] : nullptr;
}

}  // namespace

hipError_t sgemm_tier_launch(int tier, const GemmArgs& g) {
  const TierRow* t = tier_row(tier);
  if (!t || g.batch < 1) return hipErrorInvalidValue;
  if (g.ragged) {
    // one product only; a leading dimension may pad its rows, never cut them
    if (g.batch > 1) return hipErrorInvalidValue;
    if ((g.lda && g.lda < g.M) || (g.ldb && g.ldb < g.N) ||
        (g.ldc && g.ldc < g.M))
      return hipErrorInvalidValue;
    return t->launch_ragged(g);
  }
  return g.batch > 1 ? t->launch_batched(g) : t->launch(g);
}

size_t sgemm_abft_workspace_floats_ragged(int tier, int M, int N, int K) {
  const TierRow* t = tier_row(tier);
  return t && M > 0 && N > 0 && K > 0 ? t->ws_floats_ragged(M, N, K) : 0;
}

// Workspace floats needed by the fused-ABFT path of a tier (the segment-sum
// matrix SA).
size_t sgemm_abft_workspace_floats(int tier, int M, int N, int K) {
  const TierRow* t = tier_row(tier);
  return t ? t->ws_floats(M, N, K) : 0;
}

size_t sgemm_abft_workspace_floats_batched(int tier, int M, int N, int K,
                                           int nA) {
  return (nA > 0 ? (size_t)nA : 0) * sgemm_abft_workspace_floats(tier, M, N, K);
}

bool sgemm_tier_supported(int tier, int M, int N, int K) {
  const TierRow* t = tier_row(tier);
  return t && !(M % t->bm || N % t->bn || K % t->bk || M % 4 || N % 4);
}

}  // namespace ftsgemm
