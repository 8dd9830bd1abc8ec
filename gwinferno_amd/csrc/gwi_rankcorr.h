// gwi_rankcorr.h -- per-point rank (Spearman) correlations: for ONE hyper-parameter point at a time and each of two rank sets, the
// weighted second moments of the members' weighted mid-ranks (include/gwi_engine.h: gwi_set_rankcorr_columns,
// gwi_point_rank_correlations; the NumPy statement is gwinferno_amd/draws.py: rankcorr_codes, point_rank_correlations_reference; the
// contract is DESIGN 8l).  gwi_moment.h has the same second moments of the values themselves; a rank is the weighted CDF at the
// member, which changes with every point, so no per-point sum of fixed numbers gives it.
//
// The sets: kObs, all PE samples pooled (N = n_ev n_pe, member i = sample i % n_pe of event i / n_pe), u_i = w_i / S_e with w and S of
// the member's event -- one division per member, as the statement's; a per-event reciprocal would round twice -- and 0 for a member of
// a dead event; kDet, the injections, u_j = exp(lw_j - M).  What does not depend on theta is made once by the host
// (gwi_set_rankcorr_columns): per set and column the members' stable sort order and, for every member, the number of members of the
// SAME set below it (lt) and at or below it (le).  With P[c][r] the sum of u over the first r members along the order of column c and
// T_c = P[c][n], the centred mid-rank is d_ci = ((P[c][lt_i] + P[c][le_i]) - T_c) / (2 T_c) and the mid-rank r_ci = 0.5 + d_ci: ties
// share a rank, and a column whose members all tie has d = 0 and r = 0.5 exactly, whatever T_c is (the quotient is correctly
// rounded; a product with a rounded 0.5 / T_c is not exact for about one T_c in seven).
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's.  For one point draw_tile_kernel and draw_merge_kernel (unchanged) give
// every segment's maximum M and total S.  Five launches follow per point; tiles of kTile positions / samples:
//
//   rankcorr_tile_kernel     one workgroup per (set, tile of positions along the order, column): u gathered through the order, four
//                            consecutive positions per lane summed in position order, then block_inclusive_scan's total: the tile's sum
//   rankcorr_offset_kernel   one lane per (set, column) adds the tiles' sums in tile order: the tiles' exclusive offsets
//   rankcorr_prefix_kernel   the gather again and the in-tile inclusive scan in rank_prefix_kernel's fixed shape (lane order, wave scan,
//                            LDS across the four waves, no subtraction) plus the tile's offset: P[c][r + 1]; P[c][0] = 0
//   rankcorr_cov_kernel<C>   in SAMPLE order, tiles numbered as in DrawArgs, four consecutive samples per lane: per column two gathers
//                            from P, d and r; sum u, sum u r_c and sum (u d_c) d_d of every pair c <= d (each product rounded on its
//                            own) as running doubles (C is a template argument: the pairs are unrolled and stay in registers), a
//                            butterfly per item, the four waves' values through LDS and added in wave order by thread t for item t
//   rankcorr_merge_kernel    one workgroup per set: thread t adds item t over the set's tiles in tile order and divides by U = sum u;
//                            the segments' flags (hist_merge_kernel's rule on S) and the observed set's (the same rule on U)
//
// A set without weight (U is 0 or not finite) gives NaN in every slot but U.  Every sum has a fixed shape: the bits are a pure function
// of (theta, codes, masks).  No atomics, nothing depends on which workgroup arrives first, every store is a plain vector store; no
// scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace rankcorr {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxCols = 8;
constexpr int kSets = 2, kObs = 0, kDet = 1;

constexpr int pairs_of(int n_cols) { return n_cols * (n_cols + 1) / 2; }
constexpr int items_of(int n_cols) { return 1 + n_cols + pairs_of(n_cols); }  // U, the mean ranks, the upper triangle row by row

struct Args {
  draw::DrawArgs d;          // the segments, the masks, log_const, seg_max and tile_prefix of this point
  const int* order[kSets];   // [n_cols][n] per column a permutation of the set's members along which the values do not decrease
  const int* lt[kSets];      // [n_cols][n] members of the same set below the member, in [0, n]
  const int* le[kSets];      // [n_cols][n] ... at or below it
  double* prefix[kSets];     // [n_cols][n + 1]: P
  double* tile_sum;          // [n_cols][order tiles of kObs, then of kDet] the tiles' sums of u along the column's order
  double* tile_off;          // ... their exclusive prefix in tile order, per set
  double* partial;           // [n_ev * tiles_per_event + n_inj_tiles][items] the sample tiles' sums
  double* out;               // [kSets][items]: the point's row of the staging buffer
  int* dead;                 // [n_ev + 2] the segments' flags, the injection set last, then the observed set's: the point's row
  long long n[kSets];        // members: n_ev n_pe, n_inj
  int order_tiles[kSets];    // tiles along an order
  int n_cols;
};

// hist_merge_kernel's rule
__device__ inline bool live_total(double total) { return total > 0.0 && total < __builtin_inf(); }

// S of a segment as draw_merge_kernel left it
__device__ inline double total_of(const Args& a, const draw::Segment& s) { return s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0; }

// u of sample j of segment seg (an event: the observed set; n_ev: the detected set)
__device__ inline double sample_weight(const Args& a, int seg, long long j) {
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double v = draw::live_log_weight(s, j, a.d.log_const);
  if (!(v > -__builtin_inf())) return 0.0;
  const double w = exp(v - a.d.seg_max[seg]);
  if (seg == a.d.n_ev) return w;
  const double total = total_of(a, s);
  return live_total(total) ? w / total : 0.0;
}

// u of member i of a set
__device__ inline double member_weight(const Args& a, int set, long long i) {
  if (set == kDet) return sample_weight(a, a.d.n_ev, i);
  const long long ev = i / a.d.n_pe;
  return sample_weight(a, (int)ev, i - ev * a.d.n_pe);
}

// which set an order tile of the grid belongs to, and its number within the set
__device__ inline int set_of_order_tile(const Args& a, int* tile) {
  if (*tile < a.order_tiles[kObs]) return kObs;
  *tile -= a.order_tiles[kObs];
  return kDet;
}

// the weights of four consecutive positions of order tile `tile` of a set along column c's order (0 past the end)
__device__ inline void gather_tile(const Args& a, int set, int tile, int c, double (&u)[draw::kDrawPerLane]) {
  const long long n = a.n[set], start = (long long)tile * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  const int* order = a.order[set] + (long long)c * n;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) u[q] = start + q < n ? member_weight(a, set, order[start + q]) : 0.0;
}

// where the sums / offsets of a set's order tiles of column c begin
__device__ inline long long tiles_at(const Args& a, int set, int c) {
  return (long long)c * (a.order_tiles[kObs] + a.order_tiles[kDet]) + (set == kDet ? a.order_tiles[kObs] : 0);
}

__global__ __launch_bounds__(kBlock) void rankcorr_tile_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  int tile = (int)blockIdx.x;
  const int c = (int)blockIdx.y, set = set_of_order_tile(a, &tile);
  double u[draw::kDrawPerLane], run = 0.0, total;
  gather_tile(a, set, tile, c, u);
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) run += u[q];
  (void)draw::block_inclusive_scan(run, lds, &total);
  if (threadIdx.x == 0) a.tile_sum[tiles_at(a, set, c) + tile] = total;
}

__global__ __launch_bounds__(64) void rankcorr_offset_kernel(const Args a) {
  if (threadIdx.x != 0) return;  // (no barrier below)
  const int c = (int)blockIdx.x, set = (int)blockIdx.y;
  const long long at = tiles_at(a, set, c);
  double off = 0.0;
#pragma unroll 8
  for (int t = 0; t < a.order_tiles[set]; ++t) {
    a.tile_off[at + t] = off;
    off += a.tile_sum[at + t];
  }
}

__global__ __launch_bounds__(kBlock) void rankcorr_prefix_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  int tile = (int)blockIdx.x;
  const int c = (int)blockIdx.y, set = set_of_order_tile(a, &tile), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double u[draw::kDrawPerLane], run = 0.0;
  gather_tile(a, set, tile, c, u);
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) run += u[q];
  // the lanes' exclusive prefix: the wave's inclusive scan, the waves before through LDS, then the lane before (no subtraction)
  double v = run;
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  double before = 0.0;
  for (int w = 0; w < kBlock / 64; ++w)
    if (w < wave) before += lds[w];
  const double prev = __shfl_up(v, 1);
  if (lane > 0) before += prev;
  const double off = a.tile_off[tiles_at(a, set, c) + tile];
  const long long n = a.n[set], start = (long long)tile * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double* out = a.prefix[set] + (long long)c * (n + 1);
  if (tile == 0 && threadIdx.x == 0) out[0] = 0.0;
  double c_r = before;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    c_r += u[q];
    if (start + q < n) out[start + q + 1] = off + c_r;
  }
}

template <int C>
__global__ __launch_bounds__(kBlock) void rankcorr_cov_kernel(const Args a) {
  constexpr int P = pairs_of(C), kItems = items_of(C);
  __shared__ double lds[kBlock / 64][kItems];
  const int tile = (int)blockIdx.x, n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev, set = seg < a.d.n_ev ? kObs : kDet;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const long long n = a.n[set], first = set == kObs ? (long long)seg * a.d.n_pe : 0;  // the segment's first member of its set
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double t_c[C], acc[kItems];
#pragma unroll
  for (int c = 0; c < C; ++c) t_c[c] = a.prefix[set][(long long)c * (n + 1) + n];
#pragma unroll
  for (int t = 0; t < kItems; ++t) acc[t] = 0.0;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const long long j = start + q;
    const double u = j < s.n ? sample_weight(a, seg, j) : 0.0;
    if (u > 0.0) {  // (then every T_c is at least u: nothing is divided by 0)
      double d[C];
      acc[0] += u;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double* prefix = a.prefix[set] + (long long)c * (n + 1);
        const long long at = (long long)c * n + first + j;
        const double both = prefix[a.lt[set][at]] + prefix[a.le[set][at]];
        d[c] = (both - t_c[c]) / (2.0 * t_c[c]);
        acc[1 + c] += draw::scaled(u, 0.5 + d[c]);
      }
      int t = 1 + C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double ud = draw::scaled(u, d[c]);
#pragma unroll
        for (int e = c; e < C; ++e) acc[t++] += draw::scaled(ud, d[e]);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < kItems; ++t) {
    double v = acc[t];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) lds[wave][t] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < kItems) {
    double r = lds[0][threadIdx.x];
    for (int wv = 1; wv < kBlock / 64; ++wv) r += lds[wv][threadIdx.x];
    a.partial[(long long)tile * kItems + threadIdx.x] = r;
  }
  static_assert(P + C + 1 == kItems, "U, C mean ranks, P pairs");
}

__global__ __launch_bounds__(64) void rankcorr_merge_kernel(const Args a) {
  const int set = (int)blockIdx.x, t = (int)threadIdx.x, items = items_of(a.n_cols), n_ev = a.d.n_ev;
  if (set == kDet)  // the segments' flags, the injection set last
    for (int seg = t; seg <= n_ev; seg += 64) a.dead[seg] = live_total(total_of(a, draw::segment_of(a.d, seg))) ? 0 : 1;
  if (t >= items) return;  // (no barrier below)
  const int first = set == kObs ? 0 : n_ev * a.d.tiles_per_event, n_tiles = set == kObs ? n_ev * a.d.tiles_per_event : a.d.n_inj_tiles;
  const double* p = a.partial + (long long)first * items;
  double total = 0.0, sum = 0.0;  // (every thread adds U itself, in the same order: the same bits)
#pragma unroll 8
  for (int i = 0; i < n_tiles; ++i) {
    total += p[(long long)i * items];
    sum += p[(long long)i * items + t];
  }
  const bool live = live_total(total);
  if (set == kObs && t == 0) a.dead[n_ev + 1] = live ? 0 : 1;
  a.out[(long long)set * items + t] = t == 0 ? total : live ? sum / total : __builtin_nan("");
}

// rankcorr_cov_kernel<n_cols> over `tiles` tiles: the items of a kernel are unrolled, so there is one instantiation per number of columns
inline void launch_cov(unsigned tiles, hipStream_t stream, const Args& a) {
  switch (a.n_cols) {
    case 1: hipLaunchKernelGGL(rankcorr_cov_kernel<1>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 2: hipLaunchKernelGGL(rankcorr_cov_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 3: hipLaunchKernelGGL(rankcorr_cov_kernel<3>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 4: hipLaunchKernelGGL(rankcorr_cov_kernel<4>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 5: hipLaunchKernelGGL(rankcorr_cov_kernel<5>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 6: hipLaunchKernelGGL(rankcorr_cov_kernel<6>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    case 7: hipLaunchKernelGGL(rankcorr_cov_kernel<7>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
    default: hipLaunchKernelGGL(rankcorr_cov_kernel<8>, dim3(tiles), dim3(kBlock), 0, stream, a); break;
  }
}

}  // namespace rankcorr
}  // namespace gwi
