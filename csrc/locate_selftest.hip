// locate_selftest.hip — device self-test of the shared ABFT locate/correct
// (ft_kernels.hpp locate_correct).  The production injector only ever hits
// acc[0][0][0], so faults in a second fragment column (fn >= 1) or a lower
// fragment row (fm >= 1) — exactly the paths locate_correct may skip — are
// unreachable through ft_sgemm.  Here every block is ONE wave running one
// case: it synthesises a clean accumulator tile and its checksums, plants
// the case's fault(s) at arbitrary (fm, fn, reg, lane) sites, and runs both
// locate_correct and locate_correct_ref, the unscreened sweep-everything
// form it replaced.  tests/test_gpu_locate_selftest.py asserts the two are
// bit-identical and that correctable cases restore the clean tile.  The
// shipped function is driven as the fused kernels drive it: the shared
// detect (detect_partials) runs first and hands it the per-fn partials.  A
// third entry runs the detect and the screen alone and returns what they
// computed (tests/test_gpu_detect_shared.py).
#include <hip/hip_runtime.h>

#include "ft_core.h"
#include "ft_kernels.hpp"

namespace ftsgemm {
namespace {

// The locate/correct body as it stood before the per-fn screen and the
// per-fm sweep test were added: the reference the shared function must
// match bit for bit.  Kept in this TU only.
template <int FM, int FN, int MM>
__device__ inline void locate_correct_ref(
    typename mfma_traits<MM>::acc_t (&acc)[FM][FN], const float (&cc)[FN],
    const float (&cw)[FN], int sub, float tau) {
  constexpr int NREG = mfma_traits<MM>::nreg;
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    int sub_o = sub;
    asm volatile("" : "+v"(sub_o));
    double colp = 0.0;
    float colwf = 0.f;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const float v = acc[fm][fn][reg];
        colp += (double)v;
        colwf = fmaf((float)(fm * MM + acc_row(reg, sub_o)), v, colwf);
      }
    const float rc =
        (float)(dslice_sum<MM>(colp) - (double)slice_sum<MM>(cc[fn]));
    const float rw = slice_sum<MM>(colwf) - slice_sum<MM>(cw[fn]);
    const bool cbad = fabsf(rc) > tau;
    const int row = (int)rintf(rw / (cbad ? rc : 1.f));
    int sub_c = sub;
    asm volatile("" : "+v"(sub_c));
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const bool hit = cbad && (fm * MM + acc_row(reg, sub_c) == row);
        acc[fm][fn][reg] -= hit ? rc : 0.f;
      }
  }
}

// Deterministic value in (-amp, amp) from (case, element, lane).
__device__ inline float hash_val(unsigned cs, unsigned e, unsigned lane,
                                 float amp) {
  unsigned h = cs * 0x9E3779B1u ^ (e * 64u + lane) * 0x85EBCA6Bu;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  const float u = (float)(h >> 8) * (1.f / 16777216.f);  // [0, 1)
  return amp * (2.f * u - 1.f);
}

// idesc: per case 9 ints  {nfault, fm0, fn0, reg0, lane0, fm1, fn1, reg1,
//        lane1};  fdesc: per case 3 floats {mag0, mag1, tau}.
// out:   [3][ncases][FM*FN*NREG][64] = {new, ref, clean} accumulators,
//        element e = (fm*FN + fn)*NREG + reg, lane fastest.
template <int FM, int FN, int MM>
__global__ __launch_bounds__(64) void locate_selftest_kernel(
    int ncases, const int* __restrict__ idesc,
    const float* __restrict__ fdesc, float amp, float* __restrict__ out) {
  using T = mfma_traits<MM>;
  constexpr int NREG = T::nreg;
  constexpr int E = FM * FN * NREG;
  const int cs = blockIdx.x;
  if (cs >= ncases) return;
  const int lane = threadIdx.x;
  const int sub = lane / MM;

  const int* id = idesc + (size_t)cs * 9;
  const float* fd = fdesc + (size_t)cs * 3;
  const int nf = id[0];
  const float tau = fd[2];

  // One tile is live at a time (three would not fit the register file at
  // FM*FN*NREG = 128): it is refilled from the hash for each pass.  Faults
  // are planted by comparison, never by dynamic register indexing.
  typename T::acc_t tile[FM][FN];
  auto fill = [&](bool faulty) __attribute__((always_inline)) {
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) {
          float v = hash_val(cs, (fm * FN + fn) * NREG + reg, lane, amp);
          for (int f = 0; f < 2; ++f) {
            const int* s = id + 1 + 4 * f;
            if (faulty && f < nf && s[0] == fm && s[1] == fn &&
                s[2] == reg && s[3] == lane)
              v += fd[f];
          }
          tile[fm][fn][reg] = v;
        }
  };
  const size_t plane = (size_t)ncases * E * 64;
  auto store = [&](int which) __attribute__((always_inline)) {
    float* o = out + which * plane + (size_t)cs * E * 64 + lane;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg)
          o[(size_t)((fm * FN + fn) * NREG + reg) * 64] = tile[fm][fn][reg];
  };

  // clean tile -> this lane's checksum partials, in the opposite summation
  // order to the locate's own sums, so the clean residual is fp32 rounding
  // noise and not exactly zero
  fill(false);
  store(2);
  float cc[FN], cw[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    cc[fn] = 0.f;
    cw[fn] = 0.f;
#pragma unroll
    for (int fm = FM - 1; fm >= 0; --fm)
#pragma unroll
      for (int reg = NREG - 1; reg >= 0; --reg) {
        const float v = tile[fm][fn][reg];
        cc[fn] += v;
        cw[fn] = fmaf((float)(fm * MM + acc_row(reg, sub)), v, cw[fn]);
      }
  }

  // as the fused kernels do: the detect's partials feed the locate's screen
  fill(true);
  float p[FN];
  (void)detect_partials<FM, FN, MM>(tile, cc, p);
  locate_correct<FM, FN, MM>(tile, cc, cw, p, sub, tau);
  store(0);
  fill(true);
  locate_correct_ref<FM, FN, MM>(tile, cc, cw, sub, tau);
  store(1);
}

// Report variant: only the shipped locate_correct, in its fault-log (LOG)
// form, on the same case descriptors.  Every case owns a log of its own —
// counters + cs*FLOG_N_COUNTERS, events + cs*capacity*FLOG_EVENT_DWORDS —
// with the wave tile at origin (0, 0) and the k range [0, 0).
// out: [ncases][FM*FN*NREG][64], the corrected tile.
template <int FM, int FN, int MM>
__global__ __launch_bounds__(64) void locate_selftest_report_kernel(
    int ncases, const int* __restrict__ idesc,
    const float* __restrict__ fdesc, float amp, float* __restrict__ out,
    int* __restrict__ counters, int* __restrict__ events, int capacity) {
  using T = mfma_traits<MM>;
  constexpr int NREG = T::nreg;
  constexpr int E = FM * FN * NREG;
  const int cs = blockIdx.x;
  if (cs >= ncases) return;
  const int lane = threadIdx.x;
  const int sub = lane / MM;

  const int* id = idesc + (size_t)cs * 9;
  const float* fd = fdesc + (size_t)cs * 3;
  const int nf = id[0];
  const float tau = fd[2];

  typename T::acc_t tile[FM][FN];
  auto fill = [&](bool faulty) __attribute__((always_inline)) {
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) {
          float v = hash_val(cs, (fm * FN + fn) * NREG + reg, lane, amp);
          for (int f = 0; f < 2; ++f) {
            const int* s = id + 1 + 4 * f;
            if (faulty && f < nf && s[0] == fm && s[1] == fn &&
                s[2] == reg && s[3] == lane)
              v += fd[f];
          }
          tile[fm][fn][reg] = v;
        }
  };

  // same checksum construction as locate_selftest_kernel
  fill(false);
  float cc[FN], cw[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    cc[fn] = 0.f;
    cw[fn] = 0.f;
#pragma unroll
    for (int fm = FM - 1; fm >= 0; --fm)
#pragma unroll
      for (int reg = NREG - 1; reg >= 0; --reg) {
        const float v = tile[fm][fn][reg];
        cc[fn] += v;
        cw[fn] = fmaf((float)(fm * MM + acc_row(reg, sub)), v, cw[fn]);
      }
  }

  fill(true);
  FaultCtx ctx;
  ctx.log.counters = counters + (size_t)cs * FLOG_N_COUNTERS;
  ctx.log.events = events + (size_t)cs * capacity * FLOG_EVENT_DWORDS;
  ctx.log.capacity = capacity;
  float p[FN];
  (void)detect_partials<FM, FN, MM>(tile, cc, p);
  locate_correct<FM, FN, MM, true>(tile, cc, cw, p, sub, tau, ctx);
  float* o = out + (size_t)cs * E * 64 + lane;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg)
        o[(size_t)((fm * FN + fn) * NREG + reg) * 64] = tile[fm][fn][reg];
}

// Detect variant: the shared detect (detect_partials) and the locate's
// screen (screen_passes) alone, on the same case descriptors and the same
// tile and checksum construction.  Nothing is corrected.
// out: [ncases][FM*FN*NREG + 1 + 2*FN][64] floats, lane fastest: the faulty
//      tile as the detect saw it, then the residual (the same in every lane),
//      then per fn this lane's partial p[fn], then per fn 1.0 / 0.0 for a
//      screen that passed / did not (wave-uniform).
template <int FM, int FN, int MM>
__global__ __launch_bounds__(64) void detect_selftest_kernel(
    int ncases, const int* __restrict__ idesc,
    const float* __restrict__ fdesc, float amp, float* __restrict__ out) {
  using T = mfma_traits<MM>;
  constexpr int NREG = T::nreg;
  constexpr int E = FM * FN * NREG;
  constexpr int ROWS = E + 1 + 2 * FN;
  const int cs = blockIdx.x;
  if (cs >= ncases) return;
  const int lane = threadIdx.x;

  const int* id = idesc + (size_t)cs * 9;
  const float* fd = fdesc + (size_t)cs * 3;
  const int nf = id[0];
  const float tau = fd[2];

  typename T::acc_t tile[FM][FN];
  auto fill = [&](bool faulty) __attribute__((always_inline)) {
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) {
          float v = hash_val(cs, (fm * FN + fn) * NREG + reg, lane, amp);
          for (int f = 0; f < 2; ++f) {
            const int* s = id + 1 + 4 * f;
            if (faulty && f < nf && s[0] == fm && s[1] == fn &&
                s[2] == reg && s[3] == lane)
              v += fd[f];
          }
          tile[fm][fn][reg] = v;
        }
  };

  // same checksum construction as locate_selftest_kernel
  fill(false);
  float cc[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    cc[fn] = 0.f;
#pragma unroll
    for (int fm = FM - 1; fm >= 0; --fm)
#pragma unroll
      for (int reg = NREG - 1; reg >= 0; --reg) cc[fn] += tile[fm][fn][reg];
  }

  fill(true);
  float p[FN];
  const float res = detect_partials<FM, FN, MM>(tile, cc, p);
  float* o = out + (size_t)cs * ROWS * 64 + lane;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg)
        o[(size_t)((fm * FN + fn) * NREG + reg) * 64] = tile[fm][fn][reg];
  o[(size_t)E * 64] = res;
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    o[(size_t)(E + 1 + fn) * 64] = p[fn];
    o[(size_t)(E + 1 + FN + fn) * 64] =
        screen_passes<MM>(p[fn], cc[fn], tau) ? 1.f : 0.f;
  }
}

template <int FM, int FN, int MM>
hipError_t launch_detect_selftest(int ncases, const int* idesc,
                                  const float* fdesc, float amp, float* out,
                                  hipStream_t stream) {
  hipLaunchKernelGGL((detect_selftest_kernel<FM, FN, MM>), dim3(ncases),
                     dim3(64), 0, stream, ncases, idesc, fdesc, amp, out);
  return hipGetLastError();
}

template <int FM, int FN, int MM>
hipError_t launch_selftest(int ncases, const int* idesc, const float* fdesc,
                           float amp, float* out, hipStream_t stream) {
  hipLaunchKernelGGL((locate_selftest_kernel<FM, FN, MM>), dim3(ncases),
                     dim3(64), 0, stream, ncases, idesc, fdesc, amp, out);
  return hipGetLastError();
}

template <int FM, int FN, int MM>
hipError_t launch_selftest_report(int ncases, const int* idesc,
                                  const float* fdesc, float amp, float* out,
                                  int* counters, int* events, int capacity,
                                  hipStream_t stream) {
  hipLaunchKernelGGL((locate_selftest_report_kernel<FM, FN, MM>),
                     dim3(ncases), dim3(64), 0, stream, ncases, idesc, fdesc,
                     amp, out, counters, events, capacity);
  return hipGetLastError();
}

}  // namespace

hipError_t locate_selftest_report_launch(int fm, int fn, int mm, int ncases,
                                         const int* idesc, const float* fdesc,
                                         float amp, float* out, int* counters,
                                         int* events, int capacity,
                                         hipStream_t stream) {
  if (ncases < 1 || capacity < 0 || !counters || (capacity > 0 && !events))
    return hipErrorInvalidValue;
#define FT_SELFTEST_REPORT(FM_, FN_, MM_)                                    \
  if (fm == FM_ && fn == FN_ && mm == MM_)                                   \
    return launch_selftest_report<FM_, FN_, MM_>(ncases, idesc, fdesc, amp,  \
                                                 out, counters, events,      \
                                                 capacity, stream);
  FT_SELFTEST_REPORT(4, 2, 32)
  FT_SELFTEST_REPORT(2, 1, 32)
  FT_SELFTEST_REPORT(1, 2, 32)
  FT_SELFTEST_REPORT(1, 1, 32)
  FT_SELFTEST_REPORT(1, 1, 16)
#undef FT_SELFTEST_REPORT
  return hipErrorInvalidValue;
}

hipError_t detect_selftest_launch(int fm, int fn, int mm, int ncases,
                                  const int* idesc, const float* fdesc,
                                  float amp, float* out, hipStream_t stream) {
  if (ncases < 1) return hipErrorInvalidValue;
#define FT_SELFTEST_DETECT(FM_, FN_, MM_)                                   \
  if (fm == FM_ && fn == FN_ && mm == MM_)                                  \
    return launch_detect_selftest<FM_, FN_, MM_>(ncases, idesc, fdesc, amp, \
                                                 out, stream);
  FT_SELFTEST_DETECT(4, 2, 32)
  FT_SELFTEST_DETECT(2, 1, 32)
  FT_SELFTEST_DETECT(1, 2, 32)
  FT_SELFTEST_DETECT(1, 1, 32)
  FT_SELFTEST_DETECT(1, 1, 16)
#undef FT_SELFTEST_DETECT
  return hipErrorInvalidValue;
}

hipError_t locate_selftest_launch(int fm, int fn, int mm, int ncases,
                                  const int* idesc, const float* fdesc,
                                  float amp, float* out, hipStream_t stream) {
  if (ncases < 1) return hipErrorInvalidValue;
  // the wave-tile fragment shapes of the six tiers
  if (fm == 4 && fn == 2 && mm == 32)
    return launch_selftest<4, 2, 32>(ncases, idesc, fdesc, amp, out, stream);
  if (fm == 2 && fn == 1 && mm == 32)
    return launch_selftest<2, 1, 32>(ncases, idesc, fdesc, amp, out, stream);
  if (fm == 1 && fn == 2 && mm == 32)
    return launch_selftest<1, 2, 32>(ncases, idesc, fdesc, amp, out, stream);
  if (fm == 1 && fn == 1 && mm == 32)
    return launch_selftest<1, 1, 32>(ncases, idesc, fdesc, amp, out, stream);
  if (fm == 1 && fn == 1 && mm == 16)
    return launch_selftest<1, 1, 16>(ncases, idesc, fdesc, amp, out, stream);
  return hipErrorInvalidValue;
}

}  // namespace ftsgemm
