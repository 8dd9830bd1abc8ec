// gwi_mock.h -- mock catalogs: noisy data and detection of true sources, and the posterior samples of detected events
// (include/gwi_engine.h: gwi_mock_observe, gwi_mock_posteriors; the NumPy statement is gwinferno_amd/mock_catalog.py; the model is
// DESIGN.md's section "Mock catalogs").
//
// A source has C <= 8 coordinates.  Coordinate c has a transform T_c (identity or log), a noise scale sigma_c in T-space and a
// support [lo_c, hi_c] in natural units.
//
//   mock_observe_kernel    lane = source j.  d_c = T_c(x_c) + sigma_c n_c with n_c standard normal; from the DATA
//                              Mc = m1_d (1 + z_d) q_d^(3/5) / (1 + q_d)^(1/5),   rho = rho_ref (Mc / Mc_ref)^(5/6) DL_ref / DL(z_d),
//                          found = (m1_d > 0) and (q_d > 0) and (z_d > 0) and (rho >= rho_th), DL by linear interpolation in a table
//                          read from global memory (some 10^4 doubles: too large for LDS) by a binary search of at most 31 steps.
//                          rho = 0 where a detector-frame quantity is not positive or z_d lies past the table; NaN data: rho NaN,
//                          found 0.
//   mock_posterior_kernel  grid = (blocks of samples, events), lane = sample s of event e.  The posterior under a prior flat in T_c(x)
//                          on the support is a truncated normal in T-space centred on d_c: sampled by inverse CDF from ONE uniform per
//                          coordinate (no rejection loop), mapped back, clamped into the support.  prior = prod_c |T_c'(x_c)| /
//                          (T_c(hi_c) - T_c(lo_c)) at the sample.  Data that are not finite give NaN samples and a NaN prior.
//
// The generator is gwi_spinprior.h's (philox4x32_10, uniform53), key = seed.  A coordinate takes one 53-bit uniform, so Philox block b
// serves coordinates 2 b (words 0, 1) and 2 b + 1 (words 2, 3).  Counter:
//   observe:   (index low, index high, 0,        kTagObserve + b),    index = first_index + j
//   posterior: (index low, index high, sample s, kTagPosterior + b),  index = first_event + e
// kTagObserve + b and kTagPosterior + b (b < 4) are disjoint from gwi_popdraw.h's 0x504F5044, gwi_resample.h's 0x52534D50 and the
// chi_p kernel's 2 * attempt (+ 1) < 2^17.  A value is a pure function of (inputs, seed, stream index, sample index, coordinate).
//
// Inversion without cancellation.  With Phi(t) = erfc(-t / sqrt 2) / 2 for t <= 0 and Q(t) = erfc(t / sqrt 2) / 2 for t >= 0 -- erfc
// only ever of a non-negative argument -- and a, b the standardised bounds: a > 0 is mirrored (a, b, u) -> (-b, -a, 1 - u).  b <= 0:
// p = Phi(a) + u (Phi(b) - Phi(a)), y = -sqrt 2 erfcinv(2 p).  Otherwise Z = 1 - Phi(a) - Q(b); the lower branch
// y = -sqrt 2 erfcinv(2 (Phi(a) + u Z)) while that argument is <= 1, else y = +sqrt 2 erfcinv(2 (Q(b) + (1 - u) Z)); erfcinv never sees
// an argument above 1.  The noise normals use the same two branches on u and 1 - u, u = 0 read as 2^-54 (|n| < 8.3).
//
// Plain vector loads and stores, no atomics, no LDS, no scratch.  The coordinates are written out as straight-line code (a template
// over the Philox block, no loop): around a loop the compiler hoists the constants of erfcinv, erfc, log and exp out of the body and
// holds some 400 VGPRs; written out, every model entry is read at a constant offset of the kernel arguments, the roles (m1, q, z)
// are picked by comparison, and the kernels need fewer than 128 VGPRs.  Contraction is off
// wherever a value is formed that the NumPy statement forms too; erfc, erfcinv, log, exp and pow are the device library's.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_spinprior.h"

namespace gwi {
namespace mock {

constexpr int kBlock = 256;
constexpr int kMaxCoords = 8;
constexpr unsigned kTagObserve = 0x4D4F4B00u;    // counter word 3, + the block number (< 4)
constexpr unsigned kTagPosterior = 0x4D4F4B10u;  // counter word 3, + the block number (< 4)
constexpr double kSqrt2 = 1.4142135623730951, kInvSqrt2 = 0.7071067811865476;

struct Model {
  double sigma[kMaxCoords], lo[kMaxCoords], hi[kMaxCoords];
  double t_lo[kMaxCoords], t_hi[kMaxCoords], width[kMaxCoords];  // T(lo), T(hi) and T(hi) - T(lo), formed on the host
  int is_log[kMaxCoords];
  int n_coords, i_m1, i_q, i_z;
  double rho_ref, mc_ref, dl_ref, rho_th;
};

// standard normal from a uniform in [0, 1): both tails through erfcinv of an argument <= 1
__device__ inline double normal_from_uniform(double u) {
#pragma clang fp contract(off)
  if (u == 0.0) u = 5.551115123125783e-17;  // 2^-54
  return u <= 0.5 ? -kSqrt2 * erfcinv(2.0 * u) : kSqrt2 * erfcinv(2.0 * (1.0 - u));
}

// the standardised truncated normal on [a, b] at the uniform u (a <= b; NaN bounds give NaN)
__device__ inline double truncnorm_icdf(double a, double b, double u) {
#pragma clang fp contract(off)
  const bool mirror = a > 0.0;
  if (mirror) {
    const double t = a;
    a = -b;
    b = -t;
    u = 1.0 - u;
  }
  const double pa = 0.5 * erfc(-a * kInvSqrt2);
  double y;
  if (b <= 0.0) {
    const double pb = 0.5 * erfc(-b * kInvSqrt2);
    y = -kSqrt2 * erfcinv(fmin(2.0 * (pa + u * (pb - pa)), 1.0));
  } else {
    const double qb = 0.5 * erfc(b * kInvSqrt2);
    const double z = 1.0 - pa - qb;
    const double lower = 2.0 * (pa + u * z);
    if (lower <= 1.0) y = -kSqrt2 * erfcinv(lower);
    else y = kSqrt2 * erfcinv(fmin(2.0 * (qb + (1.0 - u) * z), 1.0));
  }
  if (y == y) y = fmin(fmax(y, a), b);  // (fmin / fmax would turn a NaN into a bound)
  return mirror ? -y : y;
}

// DL(z) by linear interpolation (numpy.interp's form) in the ascending table tz[0..n); z in [tz[0], tz[n - 1]]
__device__ inline double interp_table(const double* tz, const double* tv, int n, double z) {
#pragma clang fp contract(off)
  int a = 0, b = n - 1;  // tz[a] <= z, the cell is [a, a + 1]
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (tz[mid] <= z) a = mid;
    else b = mid;
  }
  const double z0 = tz[a], z1 = tz[a + 1], v0 = tv[a], v1 = tv[a + 1];
  return (v1 - v0) / (z1 - z0) * (z - z0) + v0;
}

struct ObserveArgs {
  Model m;
  const double* x;                       // [C][ld]: true parameters
  const double *table_z, *table_dl;      // [n_table]
  double* d;                             // [C][ld]
  double* snr;                           // [ld]
  unsigned char* found;                  // [ld]
  unsigned long long seed, first_index;  // first_index: the stream index of lane 0 of this launch
  long long n, ld, at;                   // lanes of this launch; row stride; position of lane 0 in the buffers
  int n_table;
};

struct Detected {
  double m1, q, z;  // T^-1 of the data of the three roles
};

template <int C>
__device__ inline void observe_coordinate(const ObserveArgs& a, long long at, double u, Detected* det) {
#pragma clang fp contract(off)
  const double x = a.x[(long long)C * a.ld + at];
  const bool is_log = a.m.is_log[C] != 0;
  const double d = (is_log ? log(x) : x) + a.m.sigma[C] * normal_from_uniform(u);
  a.d[(long long)C * a.ld + at] = d;
  const double nat = is_log ? exp(d) : d;
  if (C == a.m.i_m1) det->m1 = nat;
  if (C == a.m.i_q) det->q = nat;
  if (C == a.m.i_z) det->z = nat;
}

// Philox block B and the blocks after it: coordinates 2 B and 2 B + 1
template <int B>
__device__ inline void observe_blocks(const ObserveArgs& a, unsigned long long index, long long at, Detected* det) {
  if constexpr (2 * B < kMaxCoords) {
    if (2 * B >= a.m.n_coords) return;
    const spinprior::U4 w = spinprior::philox4x32_10(spinprior::U4{(unsigned)index, (unsigned)(index >> 32), 0u, kTagObserve + (unsigned)B}, (unsigned)a.seed, (unsigned)(a.seed >> 32));
    observe_coordinate<2 * B>(a, at, spinprior::uniform53(w.x, w.y), det);
    if (2 * B + 1 >= a.m.n_coords) return;
    observe_coordinate<2 * B + 1>(a, at, spinprior::uniform53(w.z, w.w), det);
    observe_blocks<B + 1>(a, index, at, det);
  }
}

__global__ __launch_bounds__(kBlock) void mock_observe_kernel(const ObserveArgs a) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.n) return;
  const long long at = a.at + j;
  Detected det{0.0, 0.0, 0.0};
  observe_blocks<0>(a, a.first_index + (unsigned long long)j, at, &det);
  const double m1 = det.m1, q = det.q, z = det.z;
  double rho = 0.0;
  if (!(m1 == m1) || !(q == q) || !(z == z)) {
    rho = __builtin_nan("");
  } else if (m1 > 0.0 && q > 0.0 && z > 0.0 && z <= a.table_z[a.n_table - 1] && m1 < __builtin_inf() && q < __builtin_inf()) {
    const double mc = m1 * (1.0 + z) * pow(q, 0.6) / pow(1.0 + q, 0.2);
    rho = a.m.rho_ref * pow(mc / a.m.mc_ref, 5.0 / 6.0) * a.m.dl_ref / interp_table(a.table_z, a.table_dl, a.n_table, z);
  }
  a.snr[at] = rho;
  a.found[at] = (unsigned char)(rho >= a.m.rho_th ? 1 : 0);  // (false for NaN)
}

struct PosteriorArgs {
  Model m;
  const double* d;                       // [C][n_ev]: the data of every event of the call
  double* x;                             // [C][n_ev][n_pe]
  double* prior;                         // [n_ev][n_pe]
  unsigned long long seed, first_event;  // first_event: the stream index of the call's event 0
  long long n_ev, n_pe;
  long long ev0, s0, ns;                 // this launch: event of blockIdx.y == 0, first sample, samples per event
};

template <int C>
__device__ inline void posterior_coordinate(const PosteriorArgs& a, long long e, long long at, double u, double* prior) {
#pragma clang fp contract(off)
  const double d = a.d[(long long)C * a.n_ev + e], sg = a.m.sigma[C], t_lo = a.m.t_lo[C], t_hi = a.m.t_hi[C], width = a.m.width[C];
  const bool is_log = a.m.is_log[C] != 0;
  double x = __builtin_nan("");
  if (fabs(d) < __builtin_inf()) {  // (false for NaN)
    const double y = truncnorm_icdf((t_lo - d) / sg, (t_hi - d) / sg, u);
    const double t = fmin(fmax(d + sg * y, t_lo), t_hi);
    x = fmin(fmax(is_log ? exp(t) : t, a.m.lo[C]), a.m.hi[C]);
  }
  a.x[(long long)C * (a.n_ev * a.n_pe) + at] = x;
  *prior = *prior * (is_log ? 1.0 / (x * width) : 1.0 / width);
  if (!(x == x)) *prior = x;
}

template <int B>
__device__ inline void posterior_blocks(const PosteriorArgs& a, unsigned long long index, long long e, long long s, long long at, double* prior) {
  if constexpr (2 * B < kMaxCoords) {
    if (2 * B >= a.m.n_coords) return;
    const spinprior::U4 w =
        spinprior::philox4x32_10(spinprior::U4{(unsigned)index, (unsigned)(index >> 32), (unsigned)s, kTagPosterior + (unsigned)B}, (unsigned)a.seed, (unsigned)(a.seed >> 32));
    posterior_coordinate<2 * B>(a, e, at, spinprior::uniform53(w.x, w.y), prior);
    if (2 * B + 1 >= a.m.n_coords) return;
    posterior_coordinate<2 * B + 1>(a, e, at, spinprior::uniform53(w.z, w.w), prior);
    posterior_blocks<B + 1>(a, index, e, s, at, prior);
  }
}

__global__ __launch_bounds__(kBlock) void mock_posterior_kernel(const PosteriorArgs a) {
  const long long sl = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (sl >= a.ns) return;
  const long long e = a.ev0 + blockIdx.y, s = a.s0 + sl;
  double prior = 1.0;
  posterior_blocks<0>(a, a.first_event + (unsigned long long)e, e, s, e * a.n_pe + s, &prior);
  a.prior[e * a.n_pe + s] = prior;
}

}  // namespace mock
}  // namespace gwi
