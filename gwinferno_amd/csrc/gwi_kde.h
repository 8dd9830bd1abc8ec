// gwi_kde.h -- weighted Gaussian kernel density estimates of the marginal posterior weights, in one and two dimensions: the smooth
// population-informed posterior of every event and of the predicted detected distribution, on caller-supplied grid points
// (include/gwi_engine.h: gwi_set_kde_columns, gwi_weighted_kde, gwi_weighted_kde2d; the NumPy statement is gwinferno_amd/draws.py:
// weighted_kde_reference, weighted_kde2d_reference; the contract is DESIGN 8e).
//
// Segments and tiles are gwi_draw.h's; W is the running double per sample that gwi_quant.h's marg_add_kernel leaves in HBM.  With
// p_i = W_i / sum W over a segment, s2 = sum p_i^2 and n_eff = 1 / s2, the bandwidth is scipy.stats.gaussian_kde(weights=...)'s:
// the weighted covariance sum p_i (x_i - mean)(y_i - mean_y) / (1 - s2), CENTRED on the mean of a first pass, times the square of
// the factor f = n_eff^(-1/(d+4)) (Scott) or (n_eff (d+2)/4)^(-1/(d+4)) (Silverman) times the caller's scale.  A query is
//
//   kde_moment_kernel<1>  one workgroup per tile of kDrawTile samples: the tile's sums of W, W^2, the count of samples with weight and
//                         sum W x_c of every column (four consecutive samples per lane in sample order, then draw::block_reduce)
//   kde_mean_kernel       one workgroup per segment, thread q adds quantity q over the segment's tiles in tile order: the mass, sum
//                         W^2, the count and the means
//   kde_moment_kernel<2>  the same tiles again: sum W (x_c - mean_c)^2 of every column and sum W (x - mean_x)(y - mean_y) of every pair
//   kde_band_kernel       one workgroup per segment, thread t owns column (1-D) or pair (2-D) t: the centred moments in tile order,
//                         then h (or H and its inverse), the normalising constant and the flags -- the record the evaluation reads
//   kde_eval_kernel<D>    one workgroup per (tile of samples, column or pair, block of kBlock grid points): the tile's x (and y) and W
//                         staged in LDS once, then lane l adds W_i exp(-(g - x_i)^2 / 2h^2) (D = 2: exp(-d^T H^-1 d / 2)) over the
//                         tile in sample order for ITS grid point -- every LDS read is a broadcast -- and stores one partial
//   kde_sum_kernel        one thread per (segment, column or pair, grid point): the tiles' partials in tile order, times the constant
//
// The sample chunk of an evaluation workgroup is one tile (kTile = 1 024 samples) and a grid block is kBlock = 256 points: compile-
// time constants that depend on nothing.  The partials [tiles][items][points of a pass] are bounded by the host, which cuts the grid
// blocks of a query into passes of at most kPartialCap doubles (at least one block per pass).
//
// 1-D reflection: a column with a bound lo and / or hi adds the images 2 lo - x_i and 2 hi - x_i for grid points inside [lo, hi] and
// gives 0 outside; the bandwidth is that of the unreflected data.  There is no reflection in 2-D.
//
// A segment without weight (mass 0 or not finite) gives NaN and n_eff = 0; one with fewer than two samples with weight, or whose
// variance (determinant) is not positive and finite, gives NaN and degenerate = 1.
//
// The value at a grid point is a pure function of the point, the segment's W and values and the rule: every sum has a fixed shape
// (sample order inside a tile, then tile order), a lane's arithmetic does not depend on which lane or block the point fell into, no
// atomics, nothing depends on which workgroup arrives first, every store is a plain vector store; no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_device.h"
#include "gwi_draw.h"

namespace gwi {
namespace kde {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;             // the sample chunk of one evaluation workgroup
constexpr int kMaxCols = 8;
constexpr int kMaxPairs = 4;
constexpr int kMaxGrid = 1024;                     // 1-D grid points per column
constexpr int kMaxGrid2 = 128;                     // 2-D grid points per axis
constexpr long long kPartialCap = 8ll << 20;       // doubles of evaluation partials per pass (64 MiB)
constexpr int kHead = 3;                           // per tile / segment: sum W, sum W^2, samples with weight; then per column
constexpr int kBand = 6;                           // per (segment, item): c0 c1 c2 (the exponent's coefficients), norm, state, -
constexpr double kTwoPi = 6.283185307179586476925;
enum { kLive = 0, kDead = 1, kDegenerate = 2 };    // the state of a (segment, item)
enum { kScott = 0, kSilverman = 1 };

struct Args {
  const double* w_pe;      // [n_ev][n_pe] the marginal weights
  const double* w_inj;     // [n_inj]
  const double* x_pe;      // [n_cols][n_ev][n_pe]
  const double* x_inj;     // [n_cols][n_inj]
  const double* bounds;    // [n_cols][2] reflecting bounds (NaN: none); 1-D only
  const int* pairs;        // [n_pairs][2] column indices; 2-D only
  double* part1;           // [n_tiles][kHead + n_cols], tiles numbered as in DrawArgs
  double* seg1;            // [n_ev + 1][kHead + n_cols]: mass, sum W^2, count, the means
  double* part2;           // [n_tiles][n_cols + n_pairs]
  double* band;            // [n_ev + 1][n_items][kBand]
  double* bw;              // 1-D: [n_ev + 1][n_cols] h;  2-D: [n_ev + 1][n_pairs][3] Hxx Hxy Hyy
  double* neff;            // [n_ev + 1]
  int* degenerate;         // [n_ev + 1][n_items]
  const double* gridx;     // 1-D: [n_cols][n_gx];  2-D: [n_pairs][n_gx]
  const double* gridy;     // 2-D: [n_pairs][n_gy]
  double* partial;         // [query tiles][n_items][pass_points]
  double* rho;             // [n_ev + 1][n_items][n_points]
  double scale;            // the caller's factor on f
  long long n_pe, n_inj;
  int n_ev, tiles_per_event, n_inj_tiles, n_cols, n_pairs, n_items, rule;
  int n_gx, n_gy, n_points;        // n_points = n_gx (1-D) or n_gx n_gy (2-D)
  int first_tile, first_seg;       // the launches cover tiles / segments from here on (a set without columns is left out)
  int first_block, pass_points;    // the evaluation pass: grid blocks from first_block on, pass_points points of partials per item
};

// one segment's marginal weights, its values of column 0 (column c: + c * stride) and its tiles
struct Seg {
  const double* w;
  const double* x;
  long long n, stride;
  int first_tile, n_tiles;
};

__device__ inline Seg seg_of(const Args& a, int seg) {
  if (seg < a.n_ev) return Seg{a.w_pe + (long long)seg * a.n_pe, a.x_pe + (long long)seg * a.n_pe, a.n_pe, (long long)a.n_ev * a.n_pe, seg * a.tiles_per_event, a.tiles_per_event};
  return Seg{a.w_inj, a.x_inj, a.n_inj, a.n_inj, a.n_ev * a.tiles_per_event, a.n_inj_tiles};
}

__device__ inline int seg_of_tile(const Args& a, int tile) {
  const int n_pe_tiles = a.n_ev * a.tiles_per_event;
  return tile < n_pe_tiles ? tile / a.tiles_per_event : a.n_ev;
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void kde_moment_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = a.first_tile + (int)blockIdx.x, seg = seg_of_tile(a, tile);
  const Seg s = seg_of(a, seg);
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double w[draw::kDrawPerLane];
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) w[q] = start + q < s.n ? s.w[start + q] : 0.0;
  if (PASS == 1) {
    double s0 = 0.0, s1 = 0.0, cnt = 0.0;
#pragma unroll
    for (int q = 0; q < draw::kDrawPerLane; ++q) {
      s0 += w[q];
      s1 += w[q] * w[q];
      cnt += w[q] > 0.0 ? 1.0 : 0.0;
    }
    double* out = a.part1 + (long long)tile * (kHead + a.n_cols);
    s0 = draw::block_reduce(s0, lds, draw::OpAdd());
    s1 = draw::block_reduce(s1, lds, draw::OpAdd());
    cnt = draw::block_reduce(cnt, lds, draw::OpAdd());
    if (threadIdx.x == 0) out[0] = s0, out[1] = s1, out[2] = cnt;
    for (int c = 0; c < a.n_cols; ++c) {  // (the trip count is the same for every thread)
      const double* x = s.x + (long long)c * s.stride;
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < draw::kDrawPerLane; ++q)
        if (start + q < s.n) m += w[q] * x[start + q];
      m = draw::block_reduce(m, lds, draw::OpAdd());
      if (threadIdx.x == 0) out[kHead + c] = m;
    }
  } else {
    const double* mean = a.seg1 + (long long)seg * (kHead + a.n_cols) + kHead;
    double* out = a.part2 + (long long)tile * (a.n_cols + a.n_pairs);
    for (int t = 0; t < a.n_cols + a.n_pairs; ++t) {
      const int cx = t < a.n_cols ? t : a.pairs[2 * (t - a.n_cols)], cy = t < a.n_cols ? t : a.pairs[2 * (t - a.n_cols) + 1];
      const double *x = s.x + (long long)cx * s.stride, *y = s.x + (long long)cy * s.stride;
      const double mx = mean[cx], my = mean[cy];
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < draw::kDrawPerLane; ++q)
        if (start + q < s.n) m += w[q] * (x[start + q] - mx) * (y[start + q] - my);
      m = draw::block_reduce(m, lds, draw::OpAdd());
      if (threadIdx.x == 0) out[t] = m;
    }
  }
}

__global__ __launch_bounds__(64) void kde_mean_kernel(const Args a) {
  const int seg = a.first_seg + (int)blockIdx.x, q = (int)threadIdx.x, stride = kHead + a.n_cols;
  if (q >= stride) return;
  const Seg s = seg_of(a, seg);
  const double* p = a.part1 + (long long)s.first_tile * stride + q;
  double sum = 0.0;
  for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * stride];
  // (the means divide by the mass the thread adds up itself, in the same order as thread 0: the same bits)
  if (q >= kHead) {
    const double* p0 = a.part1 + (long long)s.first_tile * stride;
    double mass = 0.0;
    for (int t = 0; t < s.n_tiles; ++t) mass += p0[(long long)t * stride];
    sum = sum / mass;
  }
  a.seg1[(long long)seg * stride + q] = sum;
}

// the factor of scipy.stats.gaussian_kde on the bandwidth, times the caller's scale
__device__ inline double factor_of(double n_eff, int d, int rule, double scale) {
  const double base = rule == kSilverman ? n_eff * (d + 2.0) / 4.0 : n_eff;
  return scale * pow(base, -1.0 / (d + 4.0));
}

template <int D>
__global__ __launch_bounds__(64) void kde_band_kernel(const Args a) {
  const int seg = a.first_seg + (int)blockIdx.x, item = (int)threadIdx.x, stride2 = a.n_cols + a.n_pairs;
  if (item >= a.n_items) return;
  const Seg s = seg_of(a, seg);
  const double* head = a.seg1 + (long long)seg * (kHead + a.n_cols);
  const double mass = head[0], sww = head[1], count = head[2], nan = __builtin_nan("");
  const double* p = a.part2 + (long long)s.first_tile * stride2;
  double* band = a.band + ((long long)seg * a.n_items + item) * kBand;
  const bool dead = !(mass > 0.0 && mass < __builtin_inf());
  const double s2 = sww / (mass * mass), n_eff = dead ? 0.0 : 1.0 / s2;
  if (item == 0) a.neff[seg] = n_eff;
  int state = dead ? kDead : count < 2.0 ? kDegenerate : kLive;
  double c0 = nan, c1 = nan, c2 = nan, norm = nan;
  if (D == 1) {
    double m = 0.0;
    for (int t = 0; t < s.n_tiles; ++t) m += p[(long long)t * stride2 + item];
    const double var = m / mass / (1.0 - s2), f = factor_of(n_eff, 1, a.rule, a.scale), h2 = var * f * f;
    if (state == kLive && !(h2 > 0.0 && h2 < __builtin_inf())) state = kDegenerate;
    if (state == kLive) {
      c0 = -0.5 / h2;
      norm = 1.0 / (mass * sqrt(kTwoPi * h2));
    }
    a.bw[(long long)seg * a.n_items + item] = state == kLive ? sqrt(h2) : nan;
  } else {
    const int cx = a.pairs[2 * item], cy = a.pairs[2 * item + 1];
    double mxx = 0.0, mxy = 0.0, myy = 0.0;
    for (int t = 0; t < s.n_tiles; ++t) {
      mxx += p[(long long)t * stride2 + cx];
      mxy += p[(long long)t * stride2 + a.n_cols + item];
      myy += p[(long long)t * stride2 + cy];
    }
    const double f = factor_of(n_eff, 2, a.rule, a.scale), k = f * f / mass / (1.0 - s2);
    const double hxx = mxx * k, hxy = mxy * k, hyy = myy * k, det = hxx * hyy - hxy * hxy;
    if (state == kLive && !(det > 0.0 && det < __builtin_inf() && hxx > 0.0 && hyy > 0.0)) state = kDegenerate;
    if (state == kLive) {  // -1/2 d^T H^-1 d = c0 dx^2 + c1 dx dy + c2 dy^2
      c0 = -0.5 * hyy / det;
      c1 = hxy / det;
      c2 = -0.5 * hxx / det;
      norm = 1.0 / (mass * kTwoPi * sqrt(det));
    }
    double* out = a.bw + ((long long)seg * a.n_items + item) * 3;
    out[0] = state == kLive ? hxx : nan;
    out[1] = state == kLive ? hxy : nan;
    out[2] = state == kLive ? hyy : nan;
  }
  band[0] = c0;
  band[1] = c1;
  band[2] = c2;
  band[3] = norm;
  band[4] = (double)state;
  band[5] = 0.0;
  a.degenerate[(long long)seg * a.n_items + item] = state == kDegenerate ? 1 : 0;
}

template <int D>
__global__ __launch_bounds__(kBlock) void kde_eval_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) double w_lds[kTile];
  __shared__ __attribute__((aligned(16))) double x_lds[kTile];
  __shared__ __attribute__((aligned(16))) double y_lds[D == 2 ? kTile : 2];
  const int tile = a.first_tile + (int)blockIdx.x, item = (int)blockIdx.y, block = a.first_block + (int)blockIdx.z;
  const int seg = seg_of_tile(a, tile);
  const double* band = a.band + ((long long)seg * a.n_items + item) * kBand;
  if (band[4] != (double)kLive) return;  // (the same for every thread; kde_sum_kernel does not read this segment's partials)
  const Seg s = seg_of(a, seg);
  const int cx = D == 2 ? a.pairs[2 * item] : item, cy = D == 2 ? a.pairs[2 * item + 1] : item;
  const double *x = s.x + (long long)cx * s.stride, *y = s.x + (long long)cy * s.stride;
  const long long tile_start = (long long)(tile - s.first_tile) * kTile;
  const int count = (int)(s.n - tile_start < kTile ? s.n - tile_start : kTile);  // (>= 1: the tile exists)
  const int j0 = (int)threadIdx.x * draw::kDrawPerLane;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const int j = j0 + q;
    const bool in = j < count;
    w_lds[j] = in ? s.w[tile_start + j] : 0.0;
    x_lds[j] = in ? x[tile_start + j] : 0.0;
    if (D == 2) y_lds[j] = in ? y[tile_start + j] : 0.0;
  }
  __syncthreads();
  const int p = block * kBlock + (int)threadIdx.x;  // this lane's grid point
  if (p >= a.n_points) return;                      // (no barrier follows)
  const double c0 = band[0], c1 = band[1], c2 = band[2];
  double acc = 0.0;
  if (D == 1) {
    const double g = a.gridx[(long long)item * a.n_gx + p];
    const double lo = a.bounds[2 * item], hi = a.bounds[2 * item + 1];
    const bool has_lo = lo == lo, has_hi = hi == hi;  // (the same for every thread)
    if (!(g < lo) && !(g > hi)) {                      // a point outside the bounds stays 0
      const double two_lo = 2.0 * lo, two_hi = 2.0 * hi;
      for (int i = 0; i < count; ++i) {
        const double w = w_lds[i], xi = x_lds[i];
        if (w > 0.0) {  // (the same for every thread)
          const double d = g - xi;
          double e = fast_exp(d * d * c0);
          if (has_lo) {
            const double dl = g - (two_lo - xi);  // (the image first, as the statement forms it: the same roundings)
            e += fast_exp(dl * dl * c0);
          }
          if (has_hi) {
            const double dh = g - (two_hi - xi);
            e += fast_exp(dh * dh * c0);
          }
          acc += w * e;
        }
      }
    }
  } else {
    const int ix = p / a.n_gy, iy = p - ix * a.n_gy;
    const double gx = a.gridx[(long long)item * a.n_gx + ix], gy = a.gridy[(long long)item * a.n_gy + iy];
    for (int i = 0; i < count; ++i) {
      const double w = w_lds[i];
      if (w > 0.0) {
        const double dx = gx - x_lds[i], dy = gy - y_lds[i];
        acc += w * fast_exp(dx * dx * c0 + dx * dy * c1 + dy * dy * c2);
      }
    }
  }
  a.partial[((long long)blockIdx.x * a.n_items + item) * a.pass_points + (p - a.first_block * kBlock)] = acc;
}

__global__ __launch_bounds__(kBlock) void kde_sum_kernel(const Args a) {
  const int seg = a.first_seg + (int)blockIdx.z, item = (int)blockIdx.y;
  const int local = (int)blockIdx.x * kBlock + (int)threadIdx.x, p = a.first_block * kBlock + local;
  if (p >= a.n_points) return;
  const Seg s = seg_of(a, seg);
  const double* band = a.band + ((long long)seg * a.n_items + item) * kBand;
  double out = __builtin_nan("");
  if (band[4] == (double)kLive) {
    const long long stride = (long long)a.n_items * a.pass_points;
    const double* part = a.partial + ((long long)(s.first_tile - a.first_tile) * a.n_items + item) * a.pass_points + local;
    double sum = 0.0;
#pragma unroll 4
    for (int t = 0; t < s.n_tiles; ++t) sum += part[(long long)t * stride];
    out = sum * band[3];
  }
  a.rho[((long long)seg * a.n_items + item) * a.n_points + p] = out;
}

}  // namespace kde
}  // namespace gwi
