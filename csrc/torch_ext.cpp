// torch_ext.cpp — PyTorch-ROCm bindings for the CDNA4 FT-SGEMM kernel
// family.  Tensor convention: a column-major MxK fp32 matrix is passed as a
// contiguous row-major (K, M) CUDA tensor (same bytes, zero copies) —
// see ft_sgemm_amd/__init__.py.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <algorithm>
#include <vector>

#include "ft_core.h"

namespace {

void check_inputs(const at::Tensor& a, const at::Tensor& b,
                  const at::Tensor& c, int64_t& M, int64_t& N, int64_t& K) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(),
              "ft_sgemm: tensors must be on a GPU device");
  TORCH_CHECK(a.scalar_type() == at::kFloat &&
                  b.scalar_type() == at::kFloat &&
                  c.scalar_type() == at::kFloat,
              "ft_sgemm: fp32 only (SGEMM)");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous() && c.is_contiguous(),
              "ft_sgemm: tensors must be contiguous");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2,
              "ft_sgemm: 2-D tensors expected");
  K = a.size(0);
  M = a.size(1);
  N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "ft_sgemm: A is (K,M) and B must be (K,N)");
  TORCH_CHECK(c.size(0) == N && c.size(1) == M,
              "ft_sgemm: C must be (N,M) for column-major MxN");
}

// The optional fault log of the fused kernels (fault_log.h) as a binding
// takes it: int32, contiguous, on the operands' device `dev`, both tensors or
// neither.  batch == 0 is an unbatched entry (sgemm, sgemm_ragged), batch >= 1
// the batched one, and the two do not accept the same sets:
//   unbatched  counters 1-D, FLOG_N_COUNTERS or more; events (capacity, 8),
//              a capacity of 0 included;
//   batched    counters exactly (batch, FLOG_N_COUNTERS); events
//              (batch, capacity, 8), capacity >= 1.
ftsgemm::FaultLog attach_fault_log(const char* nm, bool abft, at::Device dev,
                                   const c10::optional<at::Tensor>& counters,
                                   const c10::optional<at::Tensor>& events,
                                   int64_t batch) {
  TORCH_CHECK(counters.has_value() == events.has_value(), nm,
              ": fault-log counters and events go together");
  ftsgemm::FaultLog flog;
  if (!counters.has_value()) return flog;
  const at::Tensor& cn = *counters;
  const at::Tensor& ev = *events;
  const int64_t nc = ftsgemm::FLOG_N_COUNTERS, dw = ftsgemm::FLOG_EVENT_DWORDS;
  TORCH_CHECK(abft, nm, ": a fault log needs a fused-ABFT kernel");
  TORCH_CHECK(cn.scalar_type() == at::kInt && ev.scalar_type() == at::kInt,
              nm, ": fault-log tensors must be int32");
  TORCH_CHECK(cn.is_contiguous() && ev.is_contiguous(), nm,
              ": fault-log tensors must be contiguous");
  TORCH_CHECK(cn.device() == dev && ev.device() == dev, nm,
              ": fault-log tensors must be on the operands' device");
  if (batch == 0) {
    TORCH_CHECK(cn.dim() == 1 && cn.size(0) >= nc, nm,
                ": fault-log counters must hold ", nc, " int32");
    TORCH_CHECK(ev.dim() == 2 && ev.size(1) == dw && ev.size(0) <= (1 << 24),
                nm, ": fault-log events must be (capacity, ", dw, ") int32");
  } else {
    TORCH_CHECK(cn.dim() == 2 && cn.size(0) == batch && cn.size(1) == nc, nm,
                ": fault-log counters must be (batch, ", nc, ") int32");
    TORCH_CHECK(ev.dim() == 3 && ev.size(0) == batch && ev.size(2) == dw &&
                    ev.size(1) >= 1 && ev.size(1) <= (1 << 24),
                nm, ": fault-log events must be (batch, capacity, ", dw,
                ") int32");
  }
  flog.counters = cn.mutable_data_ptr<int>();
  flog.events = ev.mutable_data_ptr<int>();
  flog.capacity = (int)ev.size(-2);
  return flog;
}

// The one body behind sgemm, sgemm_batched, sgemm_ragged and
// sgemm_ragged_batched.  `g` arrives
// with the layout its entry read off the tensors (M, N, K and the batch or
// ragged fields); this fills in the rest, attaches the fault log (log_batch
// as attach_fault_log's batch), holds the call to the launch rules
// (gemm_args_error, the only statement of them on this side), allocates the
// segment-checksum scratch and launches on the current stream.
void launch_gemm(const char* nm, int64_t tier, ftsgemm::GemmArgs g, bool abft,
                 bool inject, const at::Tensor& a, const at::Tensor& b,
                 at::Tensor& c, double alpha, double beta, double tau,
                 double inj_mag, int64_t verify_windows,
                 const c10::optional<at::Tensor>& counters,
                 const c10::optional<at::Tensor>& events, int64_t log_batch) {
  const ftsgemm::FaultLog flog =
      attach_fault_log(nm, abft, a.device(), counters, events, log_batch);
  g.abft = abft, g.inject = inject;
  g.A = a.const_data_ptr<float>(), g.B = b.const_data_ptr<float>();
  g.C = c.mutable_data_ptr<float>();
  g.alpha = (float)alpha, g.beta = (float)beta;
  g.tau = (float)tau, g.inj_mag = (float)inj_mag;
  g.verify_windows = (int)verify_windows;
  g.stream = at::cuda::getCurrentCUDAStream().stream();
  g.log = flog.counters ? &flog : nullptr;
  at::Tensor ws;  // via the caching allocator; empty() launches nothing
  if (abft) {
    const size_t n = ftsgemm::sgemm_abft_workspace_floats((int)tier, g);
    ws = at::empty({(int64_t)n}, a.options());
    g.ws = ws.mutable_data_ptr<float>();
  }
  const char* broken = ftsgemm::gemm_args_error((int)tier, g);
  TORCH_CHECK(!broken, nm, ": ", broken, " (tier ", tier, ", M=", g.M,
              " N=", g.N, " K=", g.K, ")");
  hipError_t err = ftsgemm::sgemm_tier_launch((int)tier, g);
  TORCH_CHECK(err == hipSuccess, nm,
              " launch failed: ", hipGetErrorString(err));
}

// counters / events: optional fault log (attach_fault_log, unbatched form).
void sgemm(int64_t tier, bool abft, bool inject, at::Tensor a, at::Tensor b,
           at::Tensor c, double alpha, double beta, double tau,
           double inj_mag, int64_t verify_windows,
           c10::optional<at::Tensor> counters,
           c10::optional<at::Tensor> events) {
  int64_t M, N, K;
  check_inputs(a, b, c, M, N, K);
  ftsgemm::GemmArgs g{};
  g.M = (int)M, g.N = (int)N, g.K = (int)K;
  launch_gemm("ft_sgemm", tier, g, abft, inject, a, b, c, alpha, beta, tau,
              inj_mag, verify_windows, counters, events, /*log_batch=*/0);
}

// Layout of a strided-batched call, read off the tensors into the M, N, K,
// batch and stride fields of a GemmArgs: a (B,K,M), b (B,K,N), c (B,N,M),
// inner two dimensions contiguous, the batch stride whatever the tensor has.
// What a launch asks of the batch size, the strides and the alignment is
// gemm_args_error's to say (ops.batched_layout is the Python mirror that
// raises ValueError before a call gets here).
ftsgemm::GemmArgs check_batched_inputs(const at::Tensor& a,
                                       const at::Tensor& b,
                                       const at::Tensor& c) {
  const char* nm = "ft_sgemm_batched";
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), nm,
              ": tensors must be on a GPU device");
  TORCH_CHECK(a.device() == b.device() && a.device() == c.device(), nm,
              ": tensors must be on one device");
  TORCH_CHECK(a.scalar_type() == at::kFloat &&
                  b.scalar_type() == at::kFloat &&
                  c.scalar_type() == at::kFloat,
              nm, ": fp32 only (SGEMM)");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3 && c.dim() == 3, nm,
              ": 3-D tensors a (B,K,M), b (B,K,N), c (B,N,M) expected");
  const int64_t batch = c.size(0), M = a.size(2), N = b.size(2),
                K = a.size(1);
  TORCH_CHECK(a.size(0) == batch && b.size(0) == batch, nm,
              ": a, b and c must have one batch size");
  TORCH_CHECK(b.size(1) == K, nm, ": a is (B,K,M) and b must be (B,K,N)");
  TORCH_CHECK(c.size(1) == N && c.size(2) == M, nm,
              ": c must be (B,N,M) for column-major MxN");
  TORCH_CHECK(batch >= 1 && M >= 1 && N >= 1 && K >= 1, nm,
              ": empty batch or matrix");
  TORCH_CHECK(batch <= INT32_MAX && M <= INT32_MAX && N <= INT32_MAX &&
                  K <= INT32_MAX,
              nm, ": a size beyond int32");
  for (const at::Tensor* t : {&a, &b, &c})
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) == t->size(2), nm,
                ": the two inner dimensions must be contiguous");
  ftsgemm::GemmArgs g{};
  g.M = (int)M, g.N = (int)N, g.K = (int)K, g.batch = (int)batch;
  if (batch > 1)  // a single entry takes the unbatched launch: no strides
    g.strideA = a.stride(0), g.strideB = b.stride(0), g.strideC = c.stride(0);
  return g;
}

// Floats of segment-checksum scratch a fused sgemm_batched call on these
// tensors asks the allocator for: one matrix's worth when a is shared
// (batch stride 0), `batch` of them otherwise.
int64_t batched_workspace_floats(int64_t tier, const at::Tensor& a,
                                 const at::Tensor& b, const at::Tensor& c) {
  return (int64_t)ftsgemm::sgemm_abft_workspace_floats(
      (int)tier, check_batched_inputs(a, b, c));
}

// Strided-batched twin of sgemm: one launch for the whole batch.  counters
// (B, 5) / events (B, capacity, 8): one fault log per entry
// (attach_fault_log, batched form, for a batch of one as well).
void sgemm_batched(int64_t tier, bool abft, bool inject, at::Tensor a,
                   at::Tensor b, at::Tensor c, double alpha, double beta,
                   double tau, double inj_mag, int64_t verify_windows,
                   c10::optional<at::Tensor> counters,
                   c10::optional<at::Tensor> events) {
  launch_gemm("ft_sgemm_batched", tier, check_batched_inputs(a, b, c), abft,
              inject, a, b, c, alpha, beta, tau, inj_mag, verify_windows,
              counters, events, /*log_batch=*/c.size(0));
}

// Layout of a ragged call, read off the tensors into the M, N, K, ragged,
// transpose and leading-dimension fields of a GemmArgs: a (K,M), b (K,N),
// c (N,M), any sizes >= 1, unit inner stride; with trans_a, a is (M,K), with
// trans_b, b is (N,K).  The row stride is the leading dimension; a one-row
// tensor's is its width.  That it must not be shorter than the row is
// gemm_args_error's to say (ops.ragged_layout is the Python mirror that
// raises ValueError before a call gets here).
ftsgemm::GemmArgs check_ragged_inputs(const at::Tensor& a, const at::Tensor& b,
                                      const at::Tensor& c, bool trans_a,
                                      bool trans_b) {
  const char* nm = "ft_sgemm_ragged";
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), nm,
              ": tensors must be on a GPU device");
  TORCH_CHECK(a.device() == b.device() && a.device() == c.device(), nm,
              ": tensors must be on one device");
  TORCH_CHECK(a.scalar_type() == at::kFloat &&
                  b.scalar_type() == at::kFloat &&
                  c.scalar_type() == at::kFloat,
              nm, ": fp32 only (SGEMM)");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, nm,
              ": 2-D tensors a (K,M), b (K,N), c (N,M) expected");
  const int64_t M = a.size(trans_a ? 0 : 1), N = b.size(trans_b ? 0 : 1),
                K = a.size(trans_a ? 1 : 0);
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1, nm, ": empty matrix");
  TORCH_CHECK(b.size(trans_b ? 1 : 0) == K, nm,
              ": a and b disagree on K (a is (K,M), or (M,K) with trans_a; b "
              "is (K,N), or (N,K) with trans_b)");
  TORCH_CHECK(c.size(0) == N && c.size(1) == M, nm,
              ": c must be (N,M) for column-major MxN");
  TORCH_CHECK(M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX - 64, nm,
              ": a size beyond int32");
  // 0 is GemmArgs' word for packed, so a broadcast row stride of 0 must not
  // get through as a leading dimension
  const auto ld = [&](const at::Tensor& t, const char* which) {
    TORCH_CHECK(t.stride(1) == 1 || t.size(1) == 1, nm, ": ", which,
                " must have a unit inner stride");
    if (t.size(0) == 1) return (int)t.size(1);
    TORCH_CHECK(t.stride(0) >= 1 && t.stride(0) <= INT32_MAX, nm,
                ": row stride of ", which, " outside 1..2^31-1");
    return (int)t.stride(0);
  };
  ftsgemm::GemmArgs g{};
  g.M = (int)M, g.N = (int)N, g.K = (int)K;
  g.ragged = true;
  g.transA = trans_a, g.transB = trans_b;
  g.lda = ld(a, "a"), g.ldb = ld(b, "b"), g.ldc = ld(c, "c");
  return g;
}

// Ragged twin of sgemm: any M, N, K and row-strided operands, either of
// which may be given transposed.  Fault log as sgemm's.
// sk_grid > 0: the stream-K decomposition on that many workgroups, combining
// split tiles through `partials`, a contiguous fp32 tensor on the operands'
// device of at least streamk_partials_floats(tier, sk_grid) elements
// (ops.sgemm_ragged allocates it when the caller has none).  What else a
// stream-K launch asks for is gemm_args_error's to say.
void sgemm_ragged(int64_t tier, bool abft, bool inject, at::Tensor a,
                  at::Tensor b, at::Tensor c, double alpha, double beta,
                  double tau, double inj_mag, int64_t verify_windows,
                  c10::optional<at::Tensor> counters,
                  c10::optional<at::Tensor> events, bool trans_a,
                  bool trans_b, int64_t sk_grid,
                  c10::optional<at::Tensor> partials) {
  const char* nm = "ft_sgemm_ragged";
  ftsgemm::GemmArgs g = check_ragged_inputs(a, b, c, trans_a, trans_b);
  TORCH_CHECK(sk_grid >= 0 && sk_grid <= INT32_MAX, nm,
              ": sk_grid outside 0..2^31-1");
  TORCH_CHECK(sk_grid > 0 || !partials.has_value(), nm,
              ": partials go with sk_grid > 0");
  if (sk_grid > 0) {
    TORCH_CHECK(partials.has_value(), nm, ": stream-K needs partials");
    const at::Tensor& p = *partials;
    TORCH_CHECK(p.device() == a.device() && p.scalar_type() == at::kFloat &&
                    p.is_contiguous(),
                nm, ": partials must be a contiguous fp32 tensor on the "
                "operands' device");
    const size_t need =
        ftsgemm::sgemm_streamk_partials_floats((int)tier, (int)sk_grid);
    TORCH_CHECK(need == 0 || (size_t)p.numel() >= need, nm, ": partials holds ",
                p.numel(), " floats, a grid of ", sk_grid, " needs ", need);
    g.sk_grid = (int)sk_grid;
    g.sk_partials = p.mutable_data_ptr<float>();
  }
  launch_gemm(nm, tier, g, abft, inject, a, b, c, alpha, beta, tau, inj_mag,
              verify_windows, counters, events, /*log_batch=*/0);
}

// The device grid ops.sgemm_ragged(..., streamk="auto") runs on
// (sgemm_ragged_streamk_grid); 0 for a tier without a stream-K twin.
int64_t ragged_streamk_grid(int64_t tier, bool abft, bool inject, int64_t M,
                            int64_t N, int64_t K, bool trans_a,
                            bool trans_b) {
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && M <= INT32_MAX &&
                  N <= INT32_MAX && K <= INT32_MAX - 64,
              "ragged_streamk_grid: sizes outside 1..2^31-1");
  ftsgemm::GemmArgs g{};
  g.abft = abft, g.inject = inject;
  g.M = (int)M, g.N = (int)N, g.K = (int)K;
  g.ragged = true;
  g.transA = trans_a, g.transB = trans_b;
  return ftsgemm::sgemm_ragged_streamk_grid((int)tier, g);
}

int64_t streamk_partials_floats(int64_t tier, int64_t grid) {
  TORCH_CHECK(grid >= 0 && grid <= INT32_MAX,
              "streamk_partials_floats: grid outside 0..2^31-1");
  return (int64_t)ftsgemm::sgemm_streamk_partials_floats((int)tier, (int)grid);
}

int64_t ragged_workspace_floats(int64_t tier, int64_t M, int64_t N,
                                int64_t K) {
  ftsgemm::GemmArgs g{};
  g.M = (int)M, g.N = (int)N, g.K = (int)K;
  g.ragged = true;
  return (int64_t)ftsgemm::sgemm_abft_workspace_floats((int)tier, g);
}

// Layout of a strided-batched ragged call, read off the tensors: a (B,K,M),
// b (B,K,N), c (B,N,M), or a (B,M,K) with trans_a and b (B,N,K) with trans_b.
// Per entry the rules of check_ragged_inputs: unit inner stride (or inner
// size 1), the row stride is the leading dimension, a one-row tensor's is its
// width.  The batch stride is whatever the tensor has; 0 (an expand()ed
// operand) is allowed for a and b.  What a launch asks of the batch size, the
// strides and C's entries is gemm_args_error's to say
// (ops.ragged_batched_layout is the Python mirror).
ftsgemm::GemmArgs check_ragged_batched_inputs(const at::Tensor& a,
                                              const at::Tensor& b,
                                              const at::Tensor& c,
                                              bool trans_a, bool trans_b) {
  const char* nm = "ft_sgemm_ragged_batched";
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), nm,
              ": tensors must be on a GPU device");
  TORCH_CHECK(a.device() == b.device() && a.device() == c.device(), nm,
              ": tensors must be on one device");
  TORCH_CHECK(a.scalar_type() == at::kFloat &&
                  b.scalar_type() == at::kFloat &&
                  c.scalar_type() == at::kFloat,
              nm, ": fp32 only (SGEMM)");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3 && c.dim() == 3, nm,
              ": 3-D tensors a (B,K,M), b (B,K,N), c (B,N,M) expected");
  const int64_t batch = c.size(0), M = a.size(trans_a ? 1 : 2),
                N = b.size(trans_b ? 1 : 2), K = a.size(trans_a ? 2 : 1);
  TORCH_CHECK(a.size(0) == batch && b.size(0) == batch, nm,
              ": a, b and c must have one batch size");
  TORCH_CHECK(batch >= 1 && M >= 1 && N >= 1 && K >= 1, nm,
              ": empty batch or matrix");
  TORCH_CHECK(b.size(trans_b ? 2 : 1) == K, nm,
              ": a and b disagree on K (a is (B,K,M), or (B,M,K) with "
              "trans_a; b is (B,K,N), or (B,N,K) with trans_b)");
  TORCH_CHECK(c.size(1) == N && c.size(2) == M, nm,
              ": c must be (B,N,M) for column-major MxN");
  TORCH_CHECK(batch <= INT32_MAX && M <= INT32_MAX && N <= INT32_MAX &&
                  K <= INT32_MAX - 64,
              nm, ": a size beyond int32");
  const auto ld = [&](const at::Tensor& t, const char* which) {
    TORCH_CHECK(t.stride(2) == 1 || t.size(2) == 1, nm, ": ", which,
                " must have a unit inner stride");
    if (t.size(1) == 1) return (int)t.size(2);
    TORCH_CHECK(t.stride(1) >= 1 && t.stride(1) <= INT32_MAX, nm,
                ": row stride of ", which, " outside 1..2^31-1");
    return (int)t.stride(1);
  };
  ftsgemm::GemmArgs g{};
  g.M = (int)M, g.N = (int)N, g.K = (int)K, g.batch = (int)batch;
  g.ragged = true;
  g.transA = trans_a, g.transB = trans_b;
  g.lda = ld(a, "a"), g.ldb = ld(b, "b"), g.ldc = ld(c, "c");
  if (batch > 1)  // a single entry takes the single ragged launch: no strides
    g.strideA = a.stride(0), g.strideB = b.stride(0), g.strideC = c.stride(0);
  return g;
}

// Strided-batched twin of sgemm_ragged: one launch for the whole batch.
// Fault log as sgemm_batched's, one per entry.
void sgemm_ragged_batched(int64_t tier, bool abft, bool inject, at::Tensor a,
                          at::Tensor b, at::Tensor c, double alpha,
                          double beta, double tau, double inj_mag,
                          int64_t verify_windows,
                          c10::optional<at::Tensor> counters,
                          c10::optional<at::Tensor> events, bool trans_a,
                          bool trans_b) {
  launch_gemm("ft_sgemm_ragged_batched", tier,
              check_ragged_batched_inputs(a, b, c, trans_a, trans_b), abft,
              inject, a, b, c, alpha, beta, tau, inj_mag, verify_windows,
              counters, events, /*log_batch=*/c.size(0));
}

// Floats of segment-checksum scratch a fused sgemm_ragged_batched call on
// these tensors asks the allocator for: one matrix's worth when a is shared
// (batch stride 0), `batch` of them otherwise.
int64_t ragged_batched_workspace_floats(int64_t tier, const at::Tensor& a,
                                        const at::Tensor& b,
                                        const at::Tensor& c, bool trans_a,
                                        bool trans_b) {
  return (int64_t)ftsgemm::sgemm_abft_workspace_floats(
      (int)tier, check_ragged_batched_inputs(a, b, c, trans_a, trans_b));
}

// One grouped launch, planned: the per-entry problems read off three lists of
// 2-D tensors (per entry the layout of check_ragged_inputs, with empty sizes
// allowed), the descriptor table built from them and uploaded once, and the
// fused launch's workspace.  run() launches on the current stream with no
// allocation, no copy and no sync.  The plan keeps the tensors alive.
// ops.grouped_layout is the Python mirror of the rules, which
// grouped_args_error states.
//
// sk_grid: 0 plans the classic launch, G > 0 the grouped stream-K launch on
// G workgroups, -1 on the device grid (sgemm_grouped_streamk_grid).  The grid
// is clamped to the unit count and fixed for the plan, since the partials
// buffer is sized by it: `partials` (contiguous fp32 on the operands' device,
// 16-byte aligned, at least streamk_partials_floats(tier, clamped grid)
// elements) or, when none is given, a buffer the plan allocates here.  A
// group without units plans the classic launch, which launches nothing.
class GroupedPlan {
 public:
  GroupedPlan(int64_t tier, bool fused, std::vector<at::Tensor> a,
              std::vector<at::Tensor> b, std::vector<at::Tensor> c,
              bool trans_a, bool trans_b, int64_t verify_windows,
              int64_t sk_grid, c10::optional<at::Tensor> partials)
      : tier_((int)tier), a_(std::move(a)), b_(std::move(b)),
        c_(std::move(c)) {
    const char* nm = "ft_sgemm_grouped";
    TORCH_CHECK(a_.size() == c_.size() && b_.size() == c_.size(), nm,
                ": a_list, b_list and c_list must have one length");
    TORCH_CHECK(!c_.empty() && c_.size() <= (size_t)INT32_MAX, nm,
                ": empty group");
    const at::Device dev = c_[0].device();
    problems_.resize(c_.size());
    for (size_t e = 0; e < c_.size(); ++e) {
      const at::Tensor &ta = a_[e], &tb = b_[e], &tc = c_[e];
      TORCH_CHECK(ta.is_cuda() && ta.device() == dev && tb.device() == dev &&
                      tc.device() == dev,
                  nm, ": entry ", e, ": tensors must be on one GPU device");
      TORCH_CHECK(ta.scalar_type() == at::kFloat &&
                      tb.scalar_type() == at::kFloat &&
                      tc.scalar_type() == at::kFloat,
                  nm, ": entry ", e, ": fp32 only (SGEMM)");
      TORCH_CHECK(ta.dim() == 2 && tb.dim() == 2 && tc.dim() == 2, nm,
                  ": entry ", e, ": 2-D tensors expected");
      const int64_t M = ta.size(trans_a ? 0 : 1), N = tb.size(trans_b ? 0 : 1),
                    K = ta.size(trans_a ? 1 : 0);
      TORCH_CHECK(tb.size(trans_b ? 1 : 0) == K && tc.size(0) == N &&
                      tc.size(1) == M,
                  nm, ": entry ", e, ": a, b and c disagree on M, N, K");
      TORCH_CHECK(M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX - 64, nm,
                  ": entry ", e, ": a size beyond int32");
      // as check_ragged_inputs; an empty tensor is never read or written
      const auto ld = [&](const at::Tensor& t, const char* which) {
        if (t.numel() == 0) return (int)std::max<int64_t>(t.size(1), 1);
        TORCH_CHECK(t.stride(1) == 1 || t.size(1) == 1, nm, ": entry ", e,
                    ": ", which, " must have a unit inner stride");
        if (t.size(0) == 1) return (int)t.size(1);
        TORCH_CHECK(t.stride(0) >= 1 && t.stride(0) <= INT32_MAX, nm,
                    ": entry ", e, ": row stride of ", which,
                    " outside 1..2^31-1");
        return (int)t.stride(0);
      };
      ftsgemm::GroupedProblem& p = problems_[e];
      p.M = (int)M, p.N = (int)N, p.K = (int)K;
      p.lda = ld(ta, "a"), p.ldb = ld(tb, "b"), p.ldc = ld(tc, "c");
      p.A = ta.numel() ? ta.const_data_ptr<float>() : nullptr;
      p.B = tb.numel() ? tb.const_data_ptr<float>() : nullptr;
      p.C = tc.numel() ? tc.mutable_data_ptr<float>() : nullptr;
    }
    g_ = ftsgemm::GroupedArgs{};
    g_.abft = fused, g_.inject = false;
    g_.verify_windows = (int)verify_windows;
    g_.transA = trans_a, g_.transB = trans_b;
    g_.groups = (int)problems_.size();
    g_.problems = problems_.data();
    TORCH_CHECK(sk_grid >= -1 && sk_grid <= INT32_MAX, nm,
                ": sk_grid outside -1..2^31-1");
    TORCH_CHECK(sk_grid != 0 || !partials.has_value(), nm,
                ": partials go with sk_grid != 0");
    if (sk_grid != 0) {
      TORCH_CHECK(ftsgemm::sgemm_streamk_partials_floats(tier_, 1) > 0, nm,
                  ": the tier has no stream-K twin (tier ", tier, ")");
      const long long units =
          ftsgemm::sgemm_grouped_streamk_units(tier_, g_);
      TORCH_CHECK(units <= INT32_MAX, nm, ": more than 2^31 - 1 work units");
      if (sk_grid < 0) sk_grid = ftsgemm::sgemm_grouped_streamk_grid(tier_, g_);
      TORCH_CHECK(units == 0 || sk_grid > 0, nm,
                  ": no device grid for the grouped stream-K launch");
      sk_grid = std::min<int64_t>(sk_grid, units);
    }
    if (sk_grid > 0) {
      const size_t need =
          ftsgemm::sgemm_streamk_partials_floats(tier_, (int)sk_grid);
      if (partials.has_value()) {
        const at::Tensor& p = *partials;
        TORCH_CHECK(p.device() == dev && p.scalar_type() == at::kFloat &&
                        p.is_contiguous(),
                    nm, ": partials must be a contiguous fp32 tensor on the "
                    "operands' device");
        TORCH_CHECK((size_t)p.numel() >= need, nm, ": partials holds ",
                    p.numel(), " floats, a grid of ", sk_grid, " needs ", need);
        partials_ = p;
      } else {
        partials_ = at::empty({(int64_t)need}, c_[0].options());
      }
      g_.sk_grid = (int)sk_grid;
      g_.sk_partials = partials_.mutable_data_ptr<float>();
    }
    at::Tensor host = at::empty(
        {(int64_t)(g_.sk_grid > 0
                       ? ftsgemm::grouped_streamk_table_bytes(g_.groups)
                       : ftsgemm::grouped_table_bytes(g_.groups))},
        at::TensorOptions().dtype(at::kByte));
    const char* broken =
        ftsgemm::grouped_table_build(tier_, g_, host.mutable_data_ptr());
    TORCH_CHECK(!broken, nm, ": ", broken, " (tier ", tier, ", ", g_.groups,
                " entries)");
    table_ = host.to(dev);
    g_.table = table_.const_data_ptr();
    const size_t n =
        fused ? ftsgemm::sgemm_grouped_workspace_floats(tier_, g_) : 0;
    workspace_ = at::empty({(int64_t)n}, c_[0].options());
    g_.ws = n ? workspace_.mutable_data_ptr<float>() : nullptr;
  }

  at::Tensor workspace() const { return workspace_; }
  // the clamped stream-K grid (0: classic) and its partials buffer
  int64_t streamk_grid() const { return g_.sk_grid; }
  c10::optional<at::Tensor> partials() const {
    return g_.sk_grid > 0 ? c10::optional<at::Tensor>(partials_)
                          : c10::nullopt;
  }

  // counters (groups, 5) / events (groups, capacity, 8): one fault log per
  // entry (attach_fault_log, batched form).
  void run(double alpha, double beta, bool inject, double tau, double inj_mag,
           c10::optional<at::Tensor> counters,
           c10::optional<at::Tensor> events) {
    const char* nm = "ft_sgemm_grouped";
    TORCH_CHECK(g_.abft || !inject, nm, ": inject needs a fused plan");
    const ftsgemm::FaultLog flog = attach_fault_log(
        nm, g_.abft, c_[0].device(), counters, events, g_.groups);
    ftsgemm::GroupedArgs g = g_;
    g.inject = inject;
    g.alpha = (float)alpha, g.beta = (float)beta;
    g.tau = (float)tau, g.inj_mag = (float)inj_mag;
    g.stream = at::cuda::getCurrentCUDAStream().stream();
    g.log = flog.counters ? &flog : nullptr;
    // the rules were held to, with their message, when the plan was built
    hipError_t err = ftsgemm::sgemm_grouped_launch(tier_, g);
    TORCH_CHECK(err == hipSuccess, nm,
                " launch failed: ", hipGetErrorString(err));
  }

 private:
  int tier_;
  std::vector<at::Tensor> a_, b_, c_;
  std::vector<ftsgemm::GroupedProblem> problems_;
  ftsgemm::GroupedArgs g_;
  at::Tensor table_, workspace_, partials_;
};

void rocblas_sgemm_nt(at::Tensor a, at::Tensor b, at::Tensor c, double alpha,
                      double beta) {
  int64_t M, N, K;
  check_inputs(a, b, c, M, N, K);
  auto stream = at::cuda::getCurrentCUDAStream();
  int st = ftsgemm::rocblas_sgemm_nt(
      (int)M, (int)N, (int)K, a.const_data_ptr<float>(),
      b.const_data_ptr<float>(), c.mutable_data_ptr<float>(), (float)alpha,
      (float)beta, stream.stream());
  TORCH_CHECK(st == 0, "rocblas_sgemm failed with status ", st);
}

// fault: the chain's test seam (ft_core.h BaselineFault) as (panel, i, j,
// value, overwrite), validated here before anything is launched.  Returns
// (res_row, res_col, [(panel, res_row, res_col) per verified panel]).
using BaselineFaultArg =
    std::tuple<int64_t, int64_t, int64_t, double, bool>;
using BaselineVerdictRow = std::tuple<int64_t, double, double>;

std::tuple<double, double, std::vector<BaselineVerdictRow>> baseline_ft(
    at::Tensor a, at::Tensor b, at::Tensor c, double alpha, double beta,
    int64_t panel_k, c10::optional<BaselineFaultArg> fault) {
  int64_t M, N, K;
  check_inputs(a, b, c, M, N, K);
  TORCH_CHECK(panel_k >= 1, "baseline_ft: panel_k must be >= 1");
  auto opts = a.options();
  int64_t mx = std::max(M, N);
  at::Tensor ones = at::ones({mx}, opts);
  at::Tensor row_c = at::empty({M}, opts), col_c = at::empty({N}, opts);
  at::Tensor s_a = at::empty({panel_k}, opts), s_b = at::empty({panel_k}, opts);
  at::Tensor ref_row = at::empty({M}, opts), ref_col = at::empty({N}, opts);
  // one verdict slot pair per (potentially) verified panel (worst-panel
  // semantics)
  int64_t npanels = (K + panel_k - 1) / panel_k;
  at::Tensor d_res = at::empty({2 * npanels}, opts);
  ftsgemm::BaselineWorkspace ws{
      ones.mutable_data_ptr<float>(),    row_c.mutable_data_ptr<float>(),
      col_c.mutable_data_ptr<float>(),   s_a.mutable_data_ptr<float>(),
      s_b.mutable_data_ptr<float>(),     ref_row.mutable_data_ptr<float>(),
      ref_col.mutable_data_ptr<float>(), d_res.mutable_data_ptr<float>()};
  ftsgemm::BaselineFault bf{};
  if (fault.has_value()) {
    const auto& [fp, fi, fj, fv, fo] = *fault;
    TORCH_CHECK(fp >= 0 && fp < npanels, "baseline_ft: fault panel ", fp,
                " outside [0, ", npanels, ")");
    TORCH_CHECK(fi >= 0 && fi < M && fj >= 0 && fj < N,
                "baseline_ft: fault site (", fi, ", ", fj, ") outside the ", M,
                " x ", N, " result");
    bf = {(int)fp, (int)fi, (int)fj, (float)fv, fo};
  }
  float res_row = 0.f, res_col = 0.f;
  std::vector<ftsgemm::BaselineVerdict> verdicts;
  auto stream = at::cuda::getCurrentCUDAStream();
  int st = ftsgemm::baseline_ft_sgemm(
      (int)M, (int)N, (int)K, a.const_data_ptr<float>(),
      b.const_data_ptr<float>(), c.mutable_data_ptr<float>(), (float)alpha,
      (float)beta, ws, (int)panel_k, &res_row, &res_col, stream.stream(),
      fault.has_value() ? &bf : nullptr, &verdicts);
  TORCH_CHECK(st == 0, "baseline_ft_sgemm failed with status ", st);
  std::vector<BaselineVerdictRow> rows;
  for (const auto& v : verdicts)
    rows.emplace_back((int64_t)v.panel, (double)v.res_row, (double)v.res_col);
  return {(double)res_row, (double)res_col, rows};
}

bool tier_supported(int64_t tier, int64_t M, int64_t N, int64_t K) {
  return ftsgemm::sgemm_tier_supported((int)tier, (int)M, (int)N, (int)K);
}

// idesc (ncases, 9) int32 and fdesc (ncases, 3) fp32, both on a GPU — see
// ft_core.h.  Returns ncases.
int64_t check_selftest_descs(const char* name, const at::Tensor& idesc,
                             const at::Tensor& fdesc) {
  TORCH_CHECK(idesc.is_cuda() && fdesc.is_cuda(), name,
              ": descriptors must be on a GPU device");
  TORCH_CHECK(idesc.scalar_type() == at::kInt && idesc.is_contiguous() &&
                  idesc.dim() == 2 && idesc.size(1) == 9,
              name, ": idesc must be contiguous int32 (ncases, 9)");
  const int64_t ncases = idesc.size(0);
  TORCH_CHECK(fdesc.scalar_type() == at::kFloat && fdesc.is_contiguous() &&
                  fdesc.dim() == 2 && fdesc.size(0) == ncases &&
                  fdesc.size(1) == 3,
              name, ": fdesc must be contiguous fp32 (ncases, 3)");
  TORCH_CHECK(ncases >= 1 && ncases <= (1 << 20), name, ": 1..2^20 cases");
  return ncases;
}

// Checked launch arguments of a self-test entry, `out` still unset.  The
// fragment shape is range-checked here because the entries size their outputs
// from it; a shape in range that no tier has is rejected by the launch.
ftsgemm::SelftestArgs selftest_args(const char* name, int64_t fm, int64_t fn,
                                    int64_t mm, const at::Tensor& idesc,
                                    const at::Tensor& fdesc, double amp) {
  const int64_t ncases = check_selftest_descs(name, idesc, fdesc);
  TORCH_CHECK(fm >= 1 && fm <= 4 && fn >= 1 && fn <= 2 &&
                  (mm == 32 || mm == 16),
              name, ": unsupported (fm, fn, mm)");
  ftsgemm::SelftestArgs a{(int)fm, (int)fn, (int)mm, (int)ncases,
                          idesc.const_data_ptr<int>(),
                          fdesc.const_data_ptr<float>(), (float)amp};
  a.stream = at::cuda::getCurrentCUDAStream().stream();
  return a;
}

// accumulators per lane of an mm-wide MFMA fragment
int64_t nreg(int64_t mm) { return mm == 32 ? 16 : 4; }

void launch_selftest(const char* name, ftsgemm::SelftestMode mode,
                     ftsgemm::SelftestArgs& a, at::Tensor& out) {
  a.out = out.mutable_data_ptr<float>();
  hipError_t err = ftsgemm::selftest_launch(mode, a);
  TORCH_CHECK(err == hipSuccess, name, ": unsupported (fm, fn, mm) or launch "
              "failure: ", hipGetErrorString(err));
}

// Returns the (3, ncases, fm*fn*nreg, 64) {shipped, reference, clean} tiles.
at::Tensor locate_selftest(int64_t fm, int64_t fn, int64_t mm,
                           at::Tensor idesc, at::Tensor fdesc, double amp) {
  auto a = selftest_args("locate_selftest", fm, fn, mm, idesc, fdesc, amp);
  at::Tensor out = at::empty({3, a.ncases, fm * fn * nreg(mm), 64},
                             fdesc.options());
  launch_selftest("locate_selftest", ftsgemm::SELFTEST_LOCATE, a, out);
  return out;
}

// Detect variant: (ncases, fm*fn*nreg + 1 + 2*fn, 64) — the faulty tile, the
// wave residual, per fn the lane partial p[fn], per fn the screen's verdict.
at::Tensor detect_selftest(int64_t fm, int64_t fn, int64_t mm,
                           at::Tensor idesc, at::Tensor fdesc, double amp) {
  auto a = selftest_args("detect_selftest", fm, fn, mm, idesc, fdesc, amp);
  at::Tensor out = at::empty(
      {a.ncases, fm * fn * nreg(mm) + 1 + 2 * fn, 64}, fdesc.options());
  launch_selftest("detect_selftest", ftsgemm::SELFTEST_DETECT, a, out);
  return out;
}

// Report variant: (corrected tiles (ncases, fm*fn*nreg, 64), counters
// (ncases, 5) int32, events (ncases, capacity, 8) int32), one log per case.
std::tuple<at::Tensor, at::Tensor, at::Tensor> locate_selftest_report(
    int64_t fm, int64_t fn, int64_t mm, at::Tensor idesc, at::Tensor fdesc,
    double amp, int64_t capacity) {
  const char* name = "locate_selftest_report";
  auto a = selftest_args(name, fm, fn, mm, idesc, fdesc, amp);
  TORCH_CHECK(capacity >= 1 && capacity <= 1024, name, ": capacity 1..1024");
  at::Tensor out = at::empty({a.ncases, fm * fn * nreg(mm), 64},
                             fdesc.options());
  at::Tensor counters =
      at::zeros({a.ncases, ftsgemm::FLOG_N_COUNTERS}, idesc.options());
  at::Tensor events = at::zeros(
      {a.ncases, capacity, ftsgemm::FLOG_EVENT_DWORDS}, idesc.options());
  a.counters = counters.mutable_data_ptr<int>();
  a.events = events.mutable_data_ptr<int>();
  a.capacity = (int)capacity;
  launch_selftest(name, ftsgemm::SELFTEST_REPORT, a, out);
  return {out, counters, events};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sgemm", &sgemm, "tiered MFMA SGEMM (column-major C=aAB^T+bC)",
        py::arg("tier"), py::arg("abft"), py::arg("inject"), py::arg("a"),
        py::arg("b"), py::arg("c"), py::arg("alpha"), py::arg("beta"),
        py::arg("tau"), py::arg("inj_mag"), py::arg("verify_windows"),
        py::arg("counters") = py::none(), py::arg("events") = py::none());
  m.def("sgemm_batched", &sgemm_batched,
        "strided-batched tiered MFMA SGEMM, one launch per batch",
        py::arg("tier"), py::arg("abft"), py::arg("inject"), py::arg("a"),
        py::arg("b"), py::arg("c"), py::arg("alpha"), py::arg("beta"),
        py::arg("tau"), py::arg("inj_mag"), py::arg("verify_windows"),
        py::arg("counters") = py::none(), py::arg("events") = py::none());
  m.def("batched_workspace_floats", &batched_workspace_floats,
        "ABFT scratch floats a fused sgemm_batched call allocates");
  m.def("sgemm_ragged", &sgemm_ragged,
        "tiered MFMA SGEMM for any M, N, K and row-strided operands",
        py::arg("tier"), py::arg("abft"), py::arg("inject"), py::arg("a"),
        py::arg("b"), py::arg("c"), py::arg("alpha"), py::arg("beta"),
        py::arg("tau"), py::arg("inj_mag"), py::arg("verify_windows"),
        py::arg("counters") = py::none(), py::arg("events") = py::none(),
        py::arg("trans_a") = false, py::arg("trans_b") = false,
        py::arg("sk_grid") = 0, py::arg("partials") = py::none());
  m.def("ragged_workspace_floats", &ragged_workspace_floats,
        "ABFT scratch floats a fused sgemm_ragged call allocates");
  m.def("ragged_streamk_grid", &ragged_streamk_grid,
        "device grid of a ragged stream-K launch (no launch)",
        py::arg("tier"), py::arg("abft"), py::arg("inject"), py::arg("m"),
        py::arg("n"), py::arg("k"), py::arg("trans_a") = false,
        py::arg("trans_b") = false);
  m.def("streamk_partials_floats", &streamk_partials_floats,
        "floats of the partials buffer of a stream-K launch on `grid`",
        py::arg("tier"), py::arg("grid"));
  m.def("sgemm_ragged_batched", &sgemm_ragged_batched,
        "strided-batched ragged MFMA SGEMM, one launch per batch",
        py::arg("tier"), py::arg("abft"), py::arg("inject"), py::arg("a"),
        py::arg("b"), py::arg("c"), py::arg("alpha"), py::arg("beta"),
        py::arg("tau"), py::arg("inj_mag"), py::arg("verify_windows"),
        py::arg("counters") = py::none(), py::arg("events") = py::none(),
        py::arg("trans_a") = false, py::arg("trans_b") = false);
  m.def("ragged_batched_workspace_floats", &ragged_batched_workspace_floats,
        "ABFT scratch floats a fused sgemm_ragged_batched call allocates",
        py::arg("tier"), py::arg("a"), py::arg("b"), py::arg("c"),
        py::arg("trans_a") = false, py::arg("trans_b") = false);
  py::class_<GroupedPlan>(m, "GroupedPlan",
                          "descriptor table and workspace of a grouped ragged "
                          "launch, built once")
      .def(py::init<int64_t, bool, std::vector<at::Tensor>,
                    std::vector<at::Tensor>, std::vector<at::Tensor>, bool,
                    bool, int64_t, int64_t, c10::optional<at::Tensor>>(),
           py::arg("tier"), py::arg("fused"), py::arg("a_list"),
           py::arg("b_list"), py::arg("c_list"), py::arg("trans_a"),
           py::arg("trans_b"), py::arg("verify_windows"),
           py::arg("sk_grid") = 0, py::arg("partials") = py::none())
      .def_property_readonly("workspace", &GroupedPlan::workspace)
      .def_property_readonly("streamk_grid", &GroupedPlan::streamk_grid)
      .def_property_readonly("partials", &GroupedPlan::partials)
      .def("run", &GroupedPlan::run, py::arg("alpha"), py::arg("beta"),
           py::arg("inject"), py::arg("tau"), py::arg("inj_mag"),
           py::arg("counters") = py::none(), py::arg("events") = py::none());
  m.def("rocblas_sgemm", &rocblas_sgemm_nt, "rocBLAS oracle SGEMM");
  m.def("baseline_ft", &baseline_ft, "non-fused rocBLAS ABFT baseline",
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("alpha"),
        py::arg("beta"), py::arg("panel_k"), py::arg("fault") = py::none());
  m.def("tier_supported", &tier_supported, "tile divisibility check");
  m.def("locate_selftest", &locate_selftest,
        "device self-test of the ABFT locate/correct");
  m.def("detect_selftest", &detect_selftest,
        "device self-test of the shared ABFT detect and the locate's screen");
  m.def("locate_selftest_report", &locate_selftest_report,
        "self-test of the shipped locate/correct with a fault log per case");
}
