// dispatch.hip — host-side launch layer for the CDNA4 SGEMM kernel family.
// Reference-parity role: the if/else kernel dispatch of
// /root/reference/kernel/ft_sgemm/sgemm.cu:110-199, driven by the generated
// tier table; each tier's kernels live in their own translation unit
// (csrc/generated/kernel_<tier>.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

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
  hipError_t launch_tier_ragged_batched_tt_##name(const GemmArgs& g);  \
  hipError_t launch_tier_ragged_grouped_##name(const GroupedArgs& g);    \
  hipError_t launch_tier_ragged_grouped_tn_##name(const GroupedArgs& g); \
  hipError_t launch_tier_ragged_grouped_nt_##name(const GroupedArgs& g); \
  hipError_t launch_tier_ragged_grouped_tt_##name(const GroupedArgs& g);
FT_TIER_LIST(FT_DECL)
#undef FT_DECL

// ragged stream-K twins (kernel_<tier>_ragged_sk_{nn,tn,nt,tt}.hip)
#define FT_DECL_SK(name)                                         \
  hipError_t launch_tier_ragged_sk_##name(const GemmArgs& g);    \
  hipError_t launch_tier_ragged_sk_tn_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_sk_nt_##name(const GemmArgs& g); \
  hipError_t launch_tier_ragged_sk_tt_##name(const GemmArgs& g); \
  int ragged_sk_occupancy_##name(const GemmArgs& g);             \
  int ragged_sk_occupancy_tn_##name(const GemmArgs& g);          \
  int ragged_sk_occupancy_nt_##name(const GemmArgs& g);          \
  int ragged_sk_occupancy_tt_##name(const GemmArgs& g);
FT_STREAMK_TIER_LIST(FT_DECL_SK)
#undef FT_DECL_SK

// grouped ragged stream-K twins
// (kernel_<tier>_ragged_gsk_{nn,tn,nt,tt}.hip)
#define FT_DECL_GSK(name)                                                  \
  hipError_t launch_tier_ragged_grouped_sk_##name(const GroupedArgs& g);    \
  hipError_t launch_tier_ragged_grouped_sk_tn_##name(const GroupedArgs& g); \
  hipError_t launch_tier_ragged_grouped_sk_nt_##name(const GroupedArgs& g); \
  hipError_t launch_tier_ragged_grouped_sk_tt_##name(const GroupedArgs& g); \
  int ragged_grouped_sk_occupancy_##name(const GroupedArgs& g);             \
  int ragged_grouped_sk_occupancy_tn_##name(const GroupedArgs& g);          \
  int ragged_grouped_sk_occupancy_nt_##name(const GroupedArgs& g);          \
  int ragged_grouped_sk_occupancy_tt_##name(const GroupedArgs& g);
FT_STREAMK_TIER_LIST(FT_DECL_GSK)
#undef FT_DECL_GSK

namespace {

// One row per tier, in FT_TIER_LIST order: the generator numbers
// FT_TIER_ID_<name> by position in that list, so a tier id indexes the table.
struct TierRow {
  hipError_t (*launch)(const GemmArgs&);
  hipError_t (*launch_batched)(const GemmArgs&);  // batch > 1
  // g.ragged, indexed by transA + 2 * transB: one translation unit each
  hipError_t (*launch_ragged[4])(const GemmArgs&);
  hipError_t (*launch_ragged_batched[4])(const GemmArgs&);  // and batch > 1
  hipError_t (*launch_ragged_grouped[4])(const GroupedArgs&);
  int bm, bn, bk, wm;
  int bkf;  // panel depth of the fused twin
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
   {launch_tier_ragged_grouped_##name,                              \
    launch_tier_ragged_grouped_tn_##name,                           \
    launch_tier_ragged_grouped_nt_##name,                           \
    launch_tier_ragged_grouped_tt_##name},                          \
   BM, BN, BK, WM, FT_TIER_BKF_##name},
    FT_TIER_LIST(FT_ROW)
#undef FT_ROW
};

const TierRow* tier_row(int tier) {
  return tier >= 0 && tier < FT_N_TIERS ? &kTiers[tier] : nullptr;
}

// The ragged stream-K twins of a tier, indexed like launch_ragged; null rows
// for a tier without them (kernel_table.py streamk).
struct StreamkRow {
  hipError_t (*launch[4])(const GemmArgs&) = {};
  int (*occupancy[4])(const GemmArgs&) = {};
  hipError_t (*launch_grouped[4])(const GroupedArgs&) = {};
  int (*occupancy_grouped[4])(const GroupedArgs&) = {};
};
const StreamkRow* streamk_row(int tier) {
  static const StreamkRow* rows = [] {
    static StreamkRow r[FT_N_TIERS];
#define FT_SK_ROW(name)                                                 \
  r[FT_TIER_ID_##name] = StreamkRow{                                    \
      {launch_tier_ragged_sk_##name, launch_tier_ragged_sk_tn_##name,   \
       launch_tier_ragged_sk_nt_##name, launch_tier_ragged_sk_tt_##name}, \
      {ragged_sk_occupancy_##name, ragged_sk_occupancy_tn_##name,       \
       ragged_sk_occupancy_nt_##name, ragged_sk_occupancy_tt_##name},    \
      {launch_tier_ragged_grouped_sk_##name,                            \
       launch_tier_ragged_grouped_sk_tn_##name,                         \
       launch_tier_ragged_grouped_sk_nt_##name,                         \
       launch_tier_ragged_grouped_sk_tt_##name},                        \
      {ragged_grouped_sk_occupancy_##name,                              \
       ragged_grouped_sk_occupancy_tn_##name,                           \
       ragged_grouped_sk_occupancy_nt_##name,                           \
       ragged_grouped_sk_occupancy_tt_##name}};
    FT_STREAMK_TIER_LIST(FT_SK_ROW)
#undef FT_SK_ROW
    return r;
  }();
  return tier >= 0 && tier < FT_N_TIERS && rows[tier].launch[0] ? &rows[tier]
                                                                : nullptr;
}

// Work units of a ragged stream-K launch: ceil tiles x 64-k windows.
long long streamk_units(const TierRow& t, const GemmArgs& g) {
  return (long long)((g.M + t.bm - 1) / t.bm) * ((g.N + t.bn - 1) / t.bn) *
         ((g.K + 63) / 64);
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
  if (g.sk_grid < 0) return "sk_grid must be >= 0";
  if (g.sk_grid > 0) {
    if (!g.ragged || g.batch != 1)
      return "stream-K (sk_grid > 0) is for a single ragged launch";
    if (!streamk_row(tier)) return "the tier has no stream-K twin";
    if (!g.sk_partials || ((uintptr_t)g.sk_partials & 15))
      return "stream-K needs sk_partials, 16-byte aligned";
    // the unit index is an int in the kernels
    if (streamk_units(*t, g) > INT_MAX) return "more than 2^31 - 1 work units";
  }
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
    if (g.sk_grid > 0) return streamk_row(tier)->launch[tr](g);
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

int sgemm_ragged_streamk_grid(int tier, const GemmArgs& g) {
  const TierRow* t = tier_row(tier);
  const StreamkRow* sk = streamk_row(tier);
  if (!t || !sk || !g.ragged || g.batch != 1 || g.M < 1 || g.N < 1 || g.K < 1)
    return 0;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess)
    return 0;
  const int tr = (g.transA ? 1 : 0) + (g.transB ? 2 : 0);
  const long long grid = (long long)cus * sk->occupancy[tr](g);
  return (int)std::min(grid, std::min<long long>(streamk_units(*t, g), INT_MAX));
}

size_t sgemm_streamk_partials_floats(int tier, int grid) {
  const TierRow* t = tier_row(tier);
  if (!t || !streamk_row(tier) || grid < 1) return 0;
  return (size_t)2 * grid * t->bm * t->bn;
}

// ---- grouped launches (GroupedArgs) ----

namespace {

// Leading dimensions of one grouped problem with 0 resolved to packed.
struct ResolvedLd {
  int lda, ldb, ldc;
};
ResolvedLd resolve_ld(const GroupedArgs& g, const GroupedProblem& p) {
  return {p.lda ? p.lda : (g.transA ? p.K : p.M),
          p.ldb ? p.ldb : (g.transB ? p.K : p.N), p.ldc ? p.ldc : p.M};
}

bool has_sums(const GroupedProblem& p) {
  return p.M > 0 && p.N > 0 && p.K > 0;
}

// Units per tile of a grouped stream-K entry: 64-k windows, one (empty) for
// K == 0 (ft_ragged_grouped_streamk.hpp).
int grouped_upt(const GroupedProblem& p) {
  return std::max(1, (p.K + 63) / 64);
}

// Work units of a grouped stream-K launch, summed over the entries with
// tiles.
long long grouped_streamk_units(const TierRow& t, const GroupedArgs& g) {
  long long total = 0;
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    total += (long long)((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn) *
             grouped_upt(p);
  }
  return total;
}

}  // namespace

const char* grouped_args_error(int tier, const GroupedArgs& g) {
  const TierRow* t = tier_row(tier);
  if (!t) return "unknown tier id";
  if (g.groups < 1 || !g.problems) return "a grouped launch needs entries";
  long long tiles = 0;
  std::vector<std::pair<uintptr_t, uintptr_t>> spans;  // C footprints, bytes
  spans.reserve(g.groups);
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    if (p.M < 0 || p.N < 0 || p.K < 0) return "M, N and K must be >= 0";
    if (p.K > INT_MAX - 64) return "K beyond 2^31 - 65";
    if (p.M == 0 || p.N == 0) continue;  // nothing read or written
    // a leading dimension may pad its rows, never cut them; a transposed
    // operand's rows run along k
    if ((p.lda && p.lda < (g.transA ? p.K : p.M)) ||
        (p.ldb && p.ldb < (g.transB ? p.K : p.N)) || (p.ldc && p.ldc < p.M))
      return "a leading dimension is shorter than its rows";
    if (!p.C || (p.K > 0 && (!p.A || !p.B)))
      return "an entry with work needs its A, B and C";
    if (((uintptr_t)p.A | (uintptr_t)p.B | (uintptr_t)p.C) & 3)
      return "A, B and C must be 4-byte aligned";
    tiles += (long long)((p.M + t->bm - 1) / t->bm) *
             ((p.N + t->bn - 1) / t->bn);
    if (tiles > INT_MAX) return "more than 2^31 - 1 tiles";
    const long long ldc = p.ldc ? p.ldc : p.M;
    const uintptr_t c0 = (uintptr_t)p.C;
    spans.emplace_back(c0, c0 + 4 * (uintptr_t)((p.N - 1) * ldc + p.M));
  }
  // C entries are written: their footprints must be pairwise disjoint.
  // Sorted by start, each must begin where all before it have ended.
  std::sort(spans.begin(), spans.end());
  uintptr_t reach = 0;
  for (const auto& sp : spans) {
    if (sp.first < reach)
      return "C entries overlap as address intervals (entries interleaved "
             "within a row are not supported by a grouped launch)";
    reach = std::max(reach, sp.second);
  }
  if ((uintptr_t)g.ws & 3) return "ws must be 4-byte aligned";
  if (g.sk_grid < 0) return "sk_grid must be >= 0";
  if (g.sk_grid > 0) {
    if (!streamk_row(tier)) return "the tier has no stream-K twin";
    if (!g.sk_partials || ((uintptr_t)g.sk_partials & 15))
      return "stream-K needs sk_partials, 16-byte aligned";
    // the unit index is an int in the kernels
    if (grouped_streamk_units(*t, g) > INT_MAX)
      return "more than 2^31 - 1 work units";
  }
  return nullptr;
}

size_t sgemm_grouped_workspace_floats(int tier, const GroupedArgs& g) {
  const TierRow* t = tier_row(tier);
  if (!t || !g.problems) return 0;
  size_t n = 0;
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    if (has_sums(p))
      n += 2 * (size_t)((p.M + t->wm - 1) / t->wm) * abft_sstr(p.K);
  }
  return n;
}

const char* grouped_table_build(int tier, const GroupedArgs& g,
                                void* host_table) {
  if (const char* broken = grouped_args_error(tier, g)) return broken;
  const TierRow& t = kTiers[tier];
  std::memset(host_table, 0, grouped_table_bytes(g.groups));
  int* tile_start = (int*)host_table;
  GroupedEntry* entry =
      (GroupedEntry*)((char*)host_table + grouped_prefix_bytes(g.groups));
  const int bk_used = g.abft ? t.bkf : t.bk;
  int tiles = 0;
  long long ws_off = 0;
  for (int e = 0; e < g.groups; ++e) {
    const GroupedProblem& p = g.problems[e];
    const ResolvedLd ld = resolve_ld(g, p);
    GroupedEntry& d = entry[e];
    tile_start[e] = tiles;
    d.A = p.A, d.B = p.B, d.C = p.C;
    d.M = p.M, d.N = p.N, d.K = p.K;
    d.lda = ld.lda, d.ldb = ld.ldb, d.ldc = ld.ldc;
    // the 16-B paths the leading dimensions allow (RaggedFast bits 1, 2, 4);
    // the kernel clears those the entry's pointers do not (ft_ragged.hpp)
    d.fast = (ld.lda % 4 == 0 ? 1 : 0) | (ld.ldb % 4 == 0 ? 2 : 0) |
             (ld.ldc % 4 == 0 ? 4 : 0);
    d.wstride = window_stride((p.K + bk_used - 1) / bk_used,
                                      g.abft ? g.verify_windows : 1);
    d.tiles_x = (p.M + t.bm - 1) / t.bm;
    tiles += d.tiles_x * ((p.N + t.bn - 1) / t.bn);
    d.ws_off = ws_off;
    if (g.abft && has_sums(p)) {
      d.sstr = abft_sstr(p.K);
      ws_off += 2LL * ((p.M + t.wm - 1) / t.wm) * d.sstr;
    }
  }
  tile_start[g.groups] = tiles;
  if (g.sk_grid > 0) {
    // the stream-K section, behind the classic table (grouped_table.h)
    char* sec = (char*)host_table + grouped_sk_section_offset(g.groups);
    std::memset(sec, 0,
                grouped_streamk_table_bytes(g.groups) -
                    grouped_sk_section_offset(g.groups));
    int* unit_start = (int*)sec;
    int* istride = (int*)(sec + grouped_prefix_bytes(g.groups));
    long long units = 0;
    for (int e = 0; e < g.groups; ++e) {
      const GroupedProblem& p = g.problems[e];
      const int upt = grouped_upt(p);
      unit_start[e] = (int)units;
      istride[e] = window_stride(upt, g.abft ? g.verify_windows : 1);
      units += (long long)(tile_start[e + 1] - tile_start[e]) * upt;
    }
    unit_start[g.groups] = (int)units;
  }
  return nullptr;
}

hipError_t sgemm_grouped_launch(int tier, const GroupedArgs& g) {
  if (grouped_args_error(tier, g) || !g.table) return hipErrorInvalidValue;
  if (g.abft && !g.ws && sgemm_grouped_workspace_floats(tier, g) > 0)
    return hipErrorInvalidValue;
  const int tr = (g.transA ? 1 : 0) + (g.transB ? 2 : 0);
  if (g.sk_grid > 0) return streamk_row(tier)->launch_grouped[tr](g);
  return kTiers[tier].launch_ragged_grouped[tr](g);
}

long long sgemm_grouped_streamk_units(int tier, const GroupedArgs& g) {
  const TierRow* t = tier_row(tier);
  if (!t || !g.problems || g.groups < 1) return 0;
  for (int e = 0; e < g.groups; ++e)
    if (g.problems[e].M < 0 || g.problems[e].N < 0 || g.problems[e].K < 0 ||
        g.problems[e].K > INT_MAX - 64)
      return 0;
  return grouped_streamk_units(*t, g);
}

int sgemm_grouped_streamk_grid(int tier, const GroupedArgs& g) {
  const TierRow* t = tier_row(tier);
  const StreamkRow* sk = streamk_row(tier);
  if (!t || !sk) return 0;
  GroupedArgs probe = g;  // the rules without the stream-K ones
  probe.sk_grid = 0, probe.sk_partials = nullptr;
  if (grouped_args_error(tier, probe)) return 0;
  const long long units = grouped_streamk_units(*t, g);
  if (units < 1) return 0;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess)
    return 0;
  const int tr = (g.transA ? 1 : 0) + (g.transB ? 2 : 0);
  const long long grid = (long long)cus * sk->occupancy_grouped[tr](g);
  return (int)std::min(grid, std::min<long long>(units, INT_MAX));
}

}  // namespace ftsgemm
