// gwi_moment.h -- per-point first and second moments: for ONE hyper-parameter point at a time, every segment's weighted means and full
// weighted covariance of the columns of gwi_set_kde_columns (include/gwi_engine.h: gwi_point_moments; the NumPy statement is
// gwinferno_amd/draws.py: point_moments_reference; the contract is DESIGN 8j).  gwi_kde.h centres the same way, but on the marginal
// weights W summed over the points; a correlation is a ratio of centred moments and has to be taken point by point.
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's.  For one point draw_tile_kernel and draw_merge_kernel (unchanged) give
// every segment's maximum M and total S; a sample's weight is w_i = exp(lw_i - M) (0 for a sample that cannot be drawn).  With C columns
// and P = C (C + 1) / 2 pairs c <= d (upper triangle, row-major), four launches follow per point, tiles numbered as in DrawArgs:
//
//   moment_sum_kernel      one workgroup per tile: sum w x_c of every column -- four consecutive samples per lane in sample order, then
//                          draw::block_reduce
//   moment_mean_kernel     one workgroup per segment, thread c adds column c over the segment's tiles in tile order and divides by S:
//                          the means, in the point's row of the staging buffer; thread 0 stores the segment's flag
//   moment_cov_kernel<C>   the same tiles again: sum w (x_c - m_c)(x_d - m_d) of every pair, P running doubles per lane (C is a template
//                          argument: the pairs are unrolled and stay in registers), a butterfly per pair, the four waves' values through
//                          LDS and added in wave order by thread t for pair t
//   moment_merge_kernel    one workgroup per segment, thread t adds pair t over the segment's tiles in tile order and divides by S
//
// A segment without weight (S is 0 or not finite: hist_merge_kernel's rule) gives NaN and flag 1; so does, without the flag, a segment
// of a set that has no columns, which the tile launches leave out.  A segment with one live sample has w = 1 and S = 1 exactly: the
// mean is the sample and the covariance exactly 0.
//
// Every sum has a fixed shape (lane, butterfly, waves in order, tiles in order): the bits are a pure function of (theta, columns,
// masks).  No atomics, nothing depends on which workgroup arrives first, every store is a plain vector store; no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace moment {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxCols = 8;
constexpr int kMaxPairs = kMaxCols * (kMaxCols + 1) / 2;

constexpr int pairs_of(int n_cols) { return n_cols * (n_cols + 1) / 2; }

struct Args {
  draw::DrawArgs d;       // the segments, the masks, log_const, seg_max and tile_prefix of this point
  const double* x_pe;     // [n_cols][n_ev][n_pe]  (the columns of gwi_set_kde_columns; nullptr: the set has none)
  const double* x_inj;    // [n_cols][n_inj]
  double* part1;          // [n_tiles][n_cols] the tiles' sums of w x_c
  double* part2;          // [n_tiles][P] the tiles' sums of the centred products
  double* out;            // [n_ev + 1][n_cols + P] means, then the upper triangle: the point's row of the staging buffer
  int* dead;              // [n_ev + 1] the point's row of the flags' staging buffer
  int n_cols;
  int first_tile, first_seg;  // the tile launches cover tiles from here on, the columns' segments begin here (QueryCover)
  int n_seg_covered;
};

// hist_merge_kernel's rule
__device__ inline bool live_total(double total) { return total > 0.0 && total < __builtin_inf(); }

__device__ inline int seg_of_tile(const Args& a, int tile) {
  const int n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  return tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
}

// column 0 of a segment's values (column c: + c * stride)
__device__ inline const double* values_of(const Args& a, int seg, long long* stride) {
  if (seg < a.d.n_ev) {
    *stride = (long long)a.d.n_ev * a.d.n_pe;
    return a.x_pe + (long long)seg * a.d.n_pe;
  }
  *stride = a.d.n_inj;
  return a.x_inj;
}

__device__ inline bool covered(const Args& a, int seg) { return seg >= a.first_seg && seg < a.first_seg + a.n_seg_covered; }

// S of a segment as draw_merge_kernel left it
__device__ inline double total_of(const Args& a, const draw::Segment& s) { return s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0; }

// the weights of this lane's four consecutive samples of a tile (0 past the end, and for a sample that cannot be drawn)
__device__ inline void lane_weights(const Args& a, const draw::Segment& s, double big, long long start, double (&w)[draw::kDrawPerLane]) {
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    w[q] = 0.0;
    if (start + q < s.n) {
      const double v = draw::live_log_weight(s, start + q, a.d.log_const);
      if (v > -__builtin_inf()) w[q] = exp(v - big);
    }
  }
}

__global__ __launch_bounds__(kBlock) void moment_sum_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = a.first_tile + (int)blockIdx.x, seg = seg_of_tile(a, tile);
  const draw::Segment s = draw::segment_of(a.d, seg);
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  long long stride;
  const double* x0 = values_of(a, seg, &stride);
  double w[draw::kDrawPerLane];
  lane_weights(a, s, a.d.seg_max[seg], start, w);
  double* out = a.part1 + (long long)tile * a.n_cols;
  for (int c = 0; c < a.n_cols; ++c) {  // (the trip count is the same for every thread)
    const double* x = x0 + (long long)c * stride;
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < draw::kDrawPerLane; ++q)
      if (w[q] > 0.0) m += w[q] * x[start + q];
    m = draw::block_reduce(m, lds, draw::OpAdd());
    if (threadIdx.x == 0) out[c] = m;
  }
}

__global__ __launch_bounds__(64) void moment_mean_kernel(const Args a) {
  const int seg = (int)blockIdx.x, c = (int)threadIdx.x;
  if (c >= a.n_cols) return;  // (no barrier below)
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total = total_of(a, s);
  const bool live = live_total(total);
  if (c == 0) a.dead[seg] = live ? 0 : 1;
  double mean = __builtin_nan("");
  if (live && covered(a, seg)) {
    const double* p = a.part1 + (long long)s.first_tile * a.n_cols + c;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * a.n_cols];
    mean = sum / total;
  }
  a.out[(long long)seg * (a.n_cols + pairs_of(a.n_cols)) + c] = mean;
}

template <int C>
__global__ __launch_bounds__(kBlock) void moment_cov_kernel(const Args a) {
  constexpr int P = pairs_of(C);
  __shared__ double lds[kBlock / 64][P];
  const int tile = a.first_tile + (int)blockIdx.x, seg = seg_of_tile(a, tile);
  const draw::Segment s = draw::segment_of(a.d, seg);
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  long long stride;
  const double* x0 = values_of(a, seg, &stride);
  const double* mean = a.out + (long long)seg * (C + P);
  double w[draw::kDrawPerLane], m[C], acc[P];
  lane_weights(a, s, a.d.seg_max[seg], start, w);
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = mean[c];
#pragma unroll
  for (int t = 0; t < P; ++t) acc[t] = 0.0;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q)
    if (w[q] > 0.0) {
      double dx[C];
#pragma unroll
      for (int c = 0; c < C; ++c) dx[c] = x0[(long long)c * stride + start + q] - m[c];
      int t = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double wd = draw::scaled(w[q], dx[c]);
#pragma unroll
        for (int e = c; e < C; ++e) acc[t++] += draw::scaled(wd, dx[e]);
      }
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < P; ++t) {
    double v = acc[t];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) lds[wave][t] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    double r = lds[0][threadIdx.x];
    for (int wv = 1; wv < kBlock / 64; ++wv) r += lds[wv][threadIdx.x];
    a.part2[(long long)tile * P + threadIdx.x] = r;
  }
}

__global__ __launch_bounds__(64) void moment_merge_kernel(const Args a) {
  const int seg = (int)blockIdx.x, t = (int)threadIdx.x, n_pairs = pairs_of(a.n_cols);
  if (t >= n_pairs) return;  // (no barrier below)
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total = total_of(a, s);
  double v = __builtin_nan("");
  if (live_total(total) && covered(a, seg)) {
    const double* p = a.part2 + (long long)s.first_tile * n_pairs + t;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < s.n_tiles; ++i) sum += p[(long long)i * n_pairs];
    v = sum / total;
  }
  a.out[(long long)seg * (a.n_cols + n_pairs) + a.n_cols + t] = v;
}

// moment_cov_kernel<n_cols> over `tiles` tiles: the pairs of a kernel are unrolled, so there is one instantiation per number of columns
inline void launch_cov(unsigned tiles, hipStream_t stream, const Args& a) {
  switch (a.n_cols) {
    case 1: hipLaunchKernelGGL(moment_cov_kernel<1>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 2: hipLaunchKernelGGL(moment_cov_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 3: hipLaunchKernelGGL(moment_cov_kernel<3>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 4: hipLaunchKernelGGL(moment_cov_kernel<4>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 5: hipLaunchKernelGGL(moment_cov_kernel<5>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 6: hipLaunchKernelGGL(moment_cov_kernel<6>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 7: hipLaunchKernelGGL(moment_cov_kernel<7>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    default: hipLaunchKernelGGL(moment_cov_kernel<8>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
  }
}

}  // namespace moment
}  // namespace gwi
