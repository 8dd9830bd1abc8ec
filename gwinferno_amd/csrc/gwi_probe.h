// gwi_probe.h -- the device maths primitives of gwi_device.h, called on their own (include/gwi_engine.h: gwi_math_probe).  The scan
// kernels reach fast_exp, fast_rcp, the taps, the spline locators and the wave reductions only through whole terms, at the arguments
// the priors happen to produce; here one launch applies ONE primitive to caller-supplied arguments, lane by lane, so that
// tests/test_gpu_math_probe.py can hold each to a 50-digit reference (tests/golden/math_probe_hp.npz) at the edges of its domain.
// The primitives are called exactly as the scan kernels call them: nothing is copied or restated here.
//
// One workgroup of kBlock threads per kBlock lanes; lane i = blockIdx.x * kBlock + threadIdx.x.  `op` is a kernel argument, so the
// switch is wave-uniform and every lane of a wave stays active through it: the wave reductions (DPP / permlane) always see 64 live
// lanes.  A lane past n loads nothing and stores nothing, and enters a wave reduction with the op's IDENTITY -- 0 for wave_sum and
// wave_sum8, -inf for wave_max and wave_max_coarse -- so lanes past n take no part in any result.
//
// Arguments per lane i (a_stride / b_stride doubles of `a` / `b`; every lane < n stores kOutDoubles doubles and one int, unused
// slots as 0):
//   op                   a[i ...]        b[i ...]                    out[4 i ...]                        iout[i]
//   EXP                  x               -                           fast_exp(x)                         0
//   EXP_SHIFT            x               shift (whole number)        fast_exp_shift(x, shift)            0
//   EXPM1                x               -                           fast_expm1(x)                       0
//   RCP                  x               -                           fast_rcp(x)                         0
//   CUBIC_TAPS           t               -                           b0, b1, b2, b3                      0
//   CUBIC_TAPS_WEIGHTED  t               w                           w b0 ... w b3 (make_weight(w))      0
//   SPLINE_VALUE         t               coefficient c_i             spline_value at t, see below        0
//   LOCATE_KNOT          u               -                           t                                   k
//   LOCATE_TERM          u               [3]: -, -, n_basis          t                                   k
//   LOCATE_X             x               [3]: lo, inv_dx, n_basis    t                                   k
//   LOCATE               x               [3]: lo, inv_dx, n_basis    t                                   k
//   WAVE_SUM             v               -                           wave_sum over the lane's wave       0
//   WAVE_MAX             v               -                           wave_max                            0
//   WAVE_MAX_COARSE      v               -                           wave_max_coarse                     0
//   WAVE_SUM8            [8]: v[0..7]    -                           what wave_sum8(v) returns HERE      0
//   BINADES_OF           m               -                           0                                   binades_of(m)
// Every lane stores what the reduction returned to it, so lane 0's and lane 63's copies show whether the result is wave-uniform
// (wave_sum8: lanes 8k .. 8k + 7 hold the total of v[k]).
// SPLINE_VALUE follows the scan: thread tid takes b[i .. i + 3] (0 past n) as theta[tid .. tid + 3], tabulates the cubic of the knot
// interval starting at its coefficient with spline_poly into LDS at s_poly + tid, and after the barrier every lane evaluates
// spline_value at first = tid & ~3: the four lanes 4g .. 4g + 3 share the coefficients b[4g .. 4g + 3] and bring a fraction t each.
//
// Plain vector loads and stores, no atomics, no scratch, explicit arguments only (nothing read from blockDim / gridDim).
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_device.h"
#include "gwi_engine.h"

namespace gwi {
namespace probe {

constexpr int kOutDoubles = 4;

__host__ __device__ inline int a_stride(int op) { return op == GWI_PROBE_WAVE_SUM8 ? 8 : 1; }
__host__ __device__ inline int b_stride(int op) { return (op == GWI_PROBE_LOCATE_TERM || op == GWI_PROBE_LOCATE_X || op == GWI_PROBE_LOCATE) ? 3 : 1; }
__host__ __device__ inline bool uses_b(int op) {
  return op == GWI_PROBE_EXP_SHIFT || op == GWI_PROBE_CUBIC_TAPS_WEIGHTED || op == GWI_PROBE_SPLINE_VALUE || b_stride(op) == 3;
}

__global__ __launch_bounds__(kBlock) void math_probe_kernel(const int op, const long long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out,
                                                            int* __restrict__ iout) {
  __shared__ double s_poly[4 * kPolyStride];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * kBlock + tid;
  const bool live = i < n;
  const double x = live ? a[i * a_stride(op)] : 0.0;
  const double y = (live && uses_b(op)) ? b[i * b_stride(op)] : 0.0;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  int k = 0;
  switch (op) {
    case GWI_PROBE_EXP: r0 = fast_exp(x); break;
    case GWI_PROBE_EXP_SHIFT: r0 = fast_exp_shift(x, (int)y); break;
    case GWI_PROBE_EXPM1: r0 = fast_expm1(x); break;
    case GWI_PROBE_RCP: r0 = fast_rcp(x); break;
    case GWI_PROBE_CUBIC_TAPS: {
      const Taps t = cubic_taps(x);
      r0 = t.b0, r1 = t.b1, r2 = t.b2, r3 = t.b3;
      break;
    }
    case GWI_PROBE_CUBIC_TAPS_WEIGHTED: {
      const Taps t = cubic_taps_weighted(x, make_weight(y));
      r0 = t.b0, r1 = t.b1, r2 = t.b2, r3 = t.b3;
      break;
    }
    case GWI_PROBE_SPLINE_VALUE: {
      double next[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) next[j] = (i + 1 + j < n) ? b[i + 1 + j] : 0.0;
      spline_poly(y, next[0], next[1], next[2], s_poly + tid);
      __syncthreads();
      Ctx c{};
      c.poly = s_poly;
      r0 = spline_value(c, tid & ~3, x);
      break;
    }
    case GWI_PROBE_LOCATE_KNOT: spline_locate_knot(x, k, r0); break;
    case GWI_PROBE_LOCATE_TERM:
    case GWI_PROBE_LOCATE_X: {
      TermD td{};
      td.p0 = y;
      td.p2 = live ? b[i * 3 + 1] : 0.0;
      td.n_basis = live ? (int)b[i * 3 + 2] : 4;
      if (op == GWI_PROBE_LOCATE_TERM)
        spline_locate_term(x, td, k, r0);
      else
        spline_locate_x(x, td, k, r0);
      break;
    }
    case GWI_PROBE_LOCATE: spline_locate(x, y, live ? b[i * 3 + 1] : 0.0, live ? (int)b[i * 3 + 2] : 4, k, r0); break;
    case GWI_PROBE_WAVE_SUM: r0 = wave_sum(x); break;
    case GWI_PROBE_WAVE_MAX: r0 = wave_max(live ? x : GWI_NEG_INF); break;
    case GWI_PROBE_WAVE_MAX_COARSE: r0 = wave_max_coarse(live ? x : GWI_NEG_INF); break;
    case GWI_PROBE_WAVE_SUM8: {
      double v[8];
      v[0] = x;
#pragma unroll
      for (int j = 1; j < 8; ++j) v[j] = live ? a[i * 8 + j] : 0.0;
      r0 = wave_sum8(v);
      break;
    }
    case GWI_PROBE_BINADES_OF: k = binades_of(x); break;
    default: break;
  }
  if (!live) return;
  double* o = out + i * kOutDoubles;
  o[0] = r0, o[1] = r1, o[2] = r2, o[3] = r3;
  iout[i] = k;
}

}  // namespace probe
}  // namespace gwi
