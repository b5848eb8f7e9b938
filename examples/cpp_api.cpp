// C++ API example: link against the kernel TUs + dispatch + rocblas_path
// (see Makefile's `cli` target for the exact compile line).
//
//   hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -Icsrc \
//     examples/cpp_api.cpp csrc/dispatch.hip csrc/rocblas_path.hip \
//     csrc/generated/kernel_*.hip -L/opt/rocm/lib -lrocblas -o example
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "ft_core.h"
#include "generated/tile_params.h"

int main() {
  const int n = 2048;
  const size_t bytes = (size_t)n * n * sizeof(float);
  float *dA, *dB, *dC, *ws;
  hipMalloc(&dA, bytes);
  hipMalloc(&dB, bytes);
  hipMalloc(&dC, bytes);
  std::vector<float> h(n * (size_t)n, 0.5f);
  hipMemcpy(dA, h.data(), bytes, hipMemcpyHostToDevice);
  hipMemcpy(dB, h.data(), bytes, hipMemcpyHostToDevice);

  // fused-ABFT huge tier with the 20-fault self-test
  ftsgemm::GemmArgs g{/*abft=*/true, /*inject=*/true, n, n, n, dA, dB, dC,
                      /*alpha=*/1.f, /*beta=*/0.f, /*tau=*/9500.f,
                      /*inj_mag=*/10000.f, /*verify_windows=*/20};
  size_t wsf = ftsgemm::sgemm_abft_workspace_floats(FT_TIER_ID_huge, g);
  hipMalloc(&ws, wsf * sizeof(float));
  g.ws = ws;
  hipError_t err = ftsgemm::sgemm_tier_launch(FT_TIER_ID_huge, g);
  if (err != hipSuccess) {
    fprintf(stderr, "launch failed: %s\n", hipGetErrorString(err));
    return 1;
  }
  hipDeviceSynchronize();
  printf("fused-ABFT GEMM done\n");

  // the same buffers as a strided batch of four 1024^3 products, one launch:
  // A shared by every entry (strideA = 0, encoded once, so one matrix's
  // workspace is enough), B and C four consecutive 1024 x 1024 blocks
  const int nb = 1024;
  ftsgemm::GemmArgs gb{/*abft=*/true, /*inject=*/false, nb, nb, nb, dA, dB, dC,
                       1.f, 0.f, 9500.f, 10000.f, 20, ws};
  gb.batch = 4;
  gb.strideA = 0;
  gb.strideB = gb.strideC = (long long)nb * nb;
  if (ftsgemm::sgemm_abft_workspace_floats(FT_TIER_ID_huge, gb) > wsf)
    return 1;
  err = ftsgemm::sgemm_tier_launch(FT_TIER_ID_huge, gb);
  if (err != hipSuccess) {
    fprintf(stderr, "batched launch failed: %s\n", hipGetErrorString(err));
    return 1;
  }
  hipDeviceSynchronize();
  printf("strided-batched fused-ABFT GEMM done\n");

  // a 1001 x 999 x 333 sub-block of the same buffers, starting one float in
  // (4-byte alignment only) with the 2048 leading dimensions: a ragged launch
  ftsgemm::GemmArgs gr{/*abft=*/true, /*inject=*/true, 1001, 999, 333, dA + 1,
                       dB + 1, dC + 1, 1.f, 0.f, 9500.f, 10000.f, 20, ws};
  gr.ragged = true;
  gr.lda = gr.ldb = gr.ldc = n;
  if (ftsgemm::sgemm_abft_workspace_floats(FT_TIER_ID_large, gr) > wsf)
    return 1;
  err = ftsgemm::sgemm_tier_launch(FT_TIER_ID_large, gr);
  if (err != hipSuccess) {
    fprintf(stderr, "ragged launch failed: %s\n", hipGetErrorString(err));
    return 1;
  }
  hipDeviceSynchronize();
  printf("ragged fused-ABFT GEMM done\n");

  // a linear layer's forward product, y (tokens x out) = x W^T, read in
  // place: both operands are row-major with K = in as the inner dimension,
  // which is transA and transB of a ragged launch (A = W, out x in, B = x,
  // tokens x in, both with leading dimension in)
  const int tokens = 1000, in = 515, out = 777;
  ftsgemm::GemmArgs gt{/*abft=*/true, /*inject=*/true, out, tokens, in, dA,
                       dB, dC, 1.f, 0.f, 9500.f, 10000.f, 20, ws};
  gt.ragged = true;
  gt.transA = gt.transB = true;
  gt.lda = gt.ldb = in;
  if (ftsgemm::sgemm_abft_workspace_floats(FT_TIER_ID_large, gt) > wsf)
    return 1;
  err = ftsgemm::sgemm_tier_launch(FT_TIER_ID_large, gt);
  if (err != hipSuccess) {
    fprintf(stderr, "transposed launch failed: %s\n", hipGetErrorString(err));
    return 1;
  }
  hipDeviceSynchronize();
  printf("transposed ragged fused-ABFT GEMM done\n");

  // the transposes belong to ragged launches: on a tiled one the flag is
  // refused by the launch rules and nothing is launched
  ftsgemm::GemmArgs gx = g;
  gx.inject = false;
  gx.transA = true;
  const char* why = ftsgemm::gemm_args_error(FT_TIER_ID_huge, gx);
  err = ftsgemm::sgemm_tier_launch(FT_TIER_ID_huge, gx);
  if (!why || err != hipErrorInvalidValue) {
    fprintf(stderr, "a transposed tiled launch was not refused\n");
    return 1;
  }
  printf("transposed tiled launch refused: %s\n", why);
  return 0;
}
