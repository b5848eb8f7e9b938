// locate_selftest.hip — device self-test of the shared ABFT locate/correct
// (ft_kernels.hpp locate_correct).  The production injector only ever hits
// acc[0][0][0], so faults in a second fragment column (fn >= 1) or a lower
// fragment row (fm >= 1) — exactly the paths locate_correct may skip — are
// unreachable through ft_sgemm.  Here every block is ONE wave running one
// case: it synthesises a clean accumulator tile and its checksums, plants
// the case's fault(s) at arbitrary (fm, fn, reg, lane) sites, and runs both
// locate_correct and locate_correct_ref, the unscreened sweep-everything
// form it replaced.  tests/test_gpu_locate_selftest.py asserts the two are
// bit-identical and that correctable cases restore the clean tile.  A second
// mode runs the shipped function alone in its fault-log form
// (tests/test_gpu_fault_report.py); a third runs the detect and the screen
// alone and returns what they computed (tests/test_gpu_detect_shared.py).
#include <hip/hip_runtime.h>

#include <type_traits>

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

template <int V>
using int_c = std::integral_constant<int, V>;

// One case of the self-test, as every mode sees it: the decoded descriptor
// (idesc: per case 9 ints {nfault, fm0, fn0, reg0, lane0, fm1, fn1, reg1,
// lane1}; fdesc: per case 3 floats {mag0, mag1, tau}), this lane's slice of
// the synthetic FM x FN tile and its checksum partials.  One tile is live at
// a time (three would not fit the register file at FM*FN*NREG = 128): it is
// refilled from the hash for each pass.  Faults are planted by comparison,
// never by dynamic register indexing.
template <int FM, int FN, int MM>
struct SelftestCase {
  using T = mfma_traits<MM>;
  static constexpr int NREG = T::nreg;
  static constexpr int E = FM * FN * NREG;  // e = (fm*FN + fn)*NREG + reg

  int cs, lane, sub, nf;
  const int* id;
  const float* fd;
  float amp, tau;
  typename T::acc_t tile[FM][FN];
  float cc[FN], cw[FN];

  // Leaves the clean tile live and its checksum partials in cc / cw, summed
  // in the opposite order to the locate's own sums, so the clean residual is
  // fp32 rounding noise and not exactly zero.
  __device__ __forceinline__ SelftestCase(int cs_, const int* idesc,
                                          const float* fdesc, float amp_)
      : cs(cs_), lane(threadIdx.x), sub(lane / MM),
        id(idesc + (size_t)cs_ * 9), fd(fdesc + (size_t)cs_ * 3), amp(amp_) {
    nf = id[0];
    tau = fd[2];
    fill(false);
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
  }

  __device__ __forceinline__ void fill(bool faulty) {
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
  }

  // The live tile to dst[E][64], lane fastest.
  __device__ __forceinline__ void store(float* dst) const {
    float* o = dst + lane;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg)
          o[(size_t)((fm * FN + fn) * NREG + reg) * 64] = tile[fm][fn][reg];
  }
};

// One single-wave block per case; what MODE runs on the case and what it
// writes to `out` is documented at SelftestMode (ft_core.h).  Every mode
// drives the shipped code as the fused kernels do: the shared detect
// (detect_partials) runs first and hands the locate its per-fn partials.
// counters / events / capacity are read by SELFTEST_REPORT only.
template <int FM, int FN, int MM, SelftestMode MODE>
__global__ __launch_bounds__(64) void selftest_kernel(
    int ncases, const int* __restrict__ idesc,
    const float* __restrict__ fdesc, float amp, float* __restrict__ out,
    int* __restrict__ counters, int* __restrict__ events, int capacity) {
  const int cs = blockIdx.x;
  if (cs >= ncases) return;
  SelftestCase<FM, FN, MM> c(cs, idesc, fdesc, amp);
  constexpr int E = decltype(c)::E;
  float p[FN];
  if constexpr (MODE == SELFTEST_LOCATE) {
    const size_t plane = (size_t)ncases * E * 64;
    float* o = out + (size_t)cs * E * 64;
    c.store(o + 2 * plane);
    c.fill(true);
    (void)detect_partials<FM, FN, MM>(c.tile, c.cc, p);
    locate_correct<FM, FN, MM>(c.tile, c.cc, c.cw, p, c.sub, c.tau);
    c.store(o);
    c.fill(true);
    locate_correct_ref<FM, FN, MM>(c.tile, c.cc, c.cw, c.sub, c.tau);
    c.store(o + plane);
  } else if constexpr (MODE == SELFTEST_REPORT) {
    c.fill(true);
    FaultCtx ctx;
    ctx.log.counters = counters + (size_t)cs * FLOG_N_COUNTERS;
    ctx.log.events = events + (size_t)cs * capacity * FLOG_EVENT_DWORDS;
    ctx.log.capacity = capacity;
    (void)detect_partials<FM, FN, MM>(c.tile, c.cc, p);
    locate_correct<FM, FN, MM, true>(c.tile, c.cc, c.cw, p, c.sub, c.tau, ctx);
    c.store(out + (size_t)cs * E * 64);
  } else {
    c.fill(true);
    const float res = detect_partials<FM, FN, MM>(c.tile, c.cc, p);
    float* o = out + (size_t)cs * (E + 1 + 2 * FN) * 64;
    c.store(o);
    o += c.lane;
    o[(size_t)E * 64] = res;
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      o[(size_t)(E + 1 + fn) * 64] = p[fn];
      o[(size_t)(E + 1 + FN + fn) * 64] =
          screen_passes<MM>(p[fn], c.cc[fn], c.tau) ? 1.f : 0.f;
    }
  }
}

// Calls f(FM, FN, MM) as integral constants for the wave-tile fragment shape
// (fm, fn, mm) of one of the six tiers; any other shape is an error and f is
// not called.
template <class F>
hipError_t with_tile_shape(int fm, int fn, int mm, F f) {
  const auto is = [&](int a, int b, int c) {
    return fm == a && fn == b && mm == c;
  };
  if (is(4, 2, 32)) return f(int_c<4>{}, int_c<2>{}, int_c<32>{});
  if (is(2, 1, 32)) return f(int_c<2>{}, int_c<1>{}, int_c<32>{});
  if (is(1, 2, 32)) return f(int_c<1>{}, int_c<2>{}, int_c<32>{});
  if (is(1, 1, 32)) return f(int_c<1>{}, int_c<1>{}, int_c<32>{});
  if (is(1, 1, 16)) return f(int_c<1>{}, int_c<1>{}, int_c<16>{});
  return hipErrorInvalidValue;
}

template <SelftestMode MODE>
hipError_t launch_selftest(const SelftestArgs& a) {
  return with_tile_shape(a.fm, a.fn, a.mm, [&](auto FM, auto FN, auto MM) {
    hipLaunchKernelGGL((selftest_kernel<decltype(FM)::value,
                                        decltype(FN)::value,
                                        decltype(MM)::value, MODE>),
                       dim3(a.ncases), dim3(64), 0, a.stream, a.ncases,
                       a.idesc, a.fdesc, a.amp, a.out, a.counters, a.events,
                       a.capacity);
    return hipGetLastError();
  });
}

}  // namespace

hipError_t selftest_launch(SelftestMode mode, const SelftestArgs& a) {
  if (a.ncases < 1) return hipErrorInvalidValue;
  switch (mode) {
    case SELFTEST_LOCATE:
      return launch_selftest<SELFTEST_LOCATE>(a);
    case SELFTEST_REPORT:
      if (a.capacity < 0 || !a.counters || (a.capacity > 0 && !a.events))
        return hipErrorInvalidValue;
      return launch_selftest<SELFTEST_REPORT>(a);
    case SELFTEST_DETECT:
      return launch_selftest<SELFTEST_DETECT>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace ftsgemm
