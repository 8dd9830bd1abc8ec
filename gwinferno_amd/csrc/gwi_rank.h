// gwi_rank.h -- exact per-event calibration: for ONE hyper-parameter point at a time, every event's un-gridded probability integral
// transform under the predicted detected distribution, PIT = sum_i (w_i / S_e) F_det(x_i), with F_det(x) the share of detected weight
// among the injections with x_inj < x (pit_lt) or x_inj <= x (pit_le) (include/gwi_engine.h: gwi_set_rank_columns,
// gwi_point_pits_exact; the NumPy statement is gwinferno_amd/draws.py: rank_codes, point_pits_exact_reference; the contract is DESIGN
// 8i).  gwi_pit.h brackets the same number on a grid of at most 256 points; here nothing is gridded.
//
// What does not depend on theta is made once by the host (gwi_set_rank_columns): per column the injections' sort order and, for every
// PE sample, the number of injections below it (rank_lt) and at or below it (rank_le), both in [0, n_inj].  With u_j = exp(lw_j - M) the
// injections' weights at the point and P[c][r] the sum of u over the first r injections along the order of column c, F_det(x_i) is
// P[c][rank_i] / T_c with T_c = P[c][n_inj]: a device-wide prefix in sort order and two gathers per PE sample and column.
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's.  For one point draw_tile_kernel and draw_merge_kernel (unchanged) give
// every segment's maximum M and total S.  Five launches follow per point, tiles of kTile ranks / samples numbered as in DrawArgs:
//
//   rank_tile_kernel       one workgroup per (injection tile, column): the injections' weights gathered through the order, four
//                          consecutive ranks per lane summed in rank order, then block_inclusive_scan's total: the tile's sum
//   rank_merge_kernel      one workgroup per column: the tiles' exclusive offsets, one lane adding the sums in tile order
//   rank_prefix_kernel     one workgroup per (injection tile, column): the gather again and the in-tile inclusive scan -- lane order,
//                          wave scan, LDS across the four waves, as quant_select_kernel's -- plus the tile's offset: P[c][r + 1]; the
//                          first workgroup of a column stores P[c][0] = 0
//   pit_rank_kernel        one workgroup per (event tile, column): four consecutive samples per lane, sum_i w_i P[c][rank_lt_i] and
//                          sum_i w_i P[c][rank_le_i] (each product rounded on its own) summed in sample order, then block_reduce: two
//                          doubles per (tile, column)
//   pit_rank_merge_kernel  one workgroup per (event, column): one lane adds the tiles' partial sums in tile order and forms
//                          pit = sum / S_e / T_c, two divisions in that order; NaN for a dead event or a dead injection segment (S or
//                          T is 0 or not finite: hist_merge_kernel's rule); thread 0 of column 0 stores the segment's flag, and the
//                          last row of workgroups that of the injection segment
//
// Every sum has a fixed shape: the bits are a pure function of (theta, ranks, masks).  No atomics, nothing depends on which workgroup
// arrives first, every store is a plain vector store; no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace rank {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxCols = 8;

struct Args {
  draw::DrawArgs d;       // the segments, the masks, log_const, seg_max and tile_prefix of this point
  const int* order_inj;   // [n_cols][n_inj] per column a permutation of 0 ... n_inj - 1 along which the values do not decrease
  const int* rank_lt;     // [n_cols][n_ev][n_pe] injections below the sample, in [0, n_inj]
  const int* rank_le;     // [n_cols][n_ev][n_pe] ... at or below it
  double* tile_sum;       // [n_cols][n_inj_tiles] the injection tiles' sums of u along the column's order
  double* tile_off;       // [n_cols][n_inj_tiles] ... their exclusive prefix in tile order
  double* prefix;         // [n_cols][n_inj + 1]: P
  double* partial;        // [n_ev * tiles_per_event][n_cols][2] the event tiles' partial sums (lt, le)
  double* pit;            // [n_ev][n_cols][2] (lt, le): the point's row of the staging buffer
  int* dead;              // [n_ev + 1] the point's row of the flags' staging buffer
  int n_cols;
};

// hist_merge_kernel's rule
__device__ inline bool live_total(double total) { return total > 0.0 && total < __builtin_inf(); }

// the weights of four consecutive ranks of injection tile `tile` along column c's order (0 past the end, and for a sample without weight)
__device__ inline void gather_tile(const Args& a, const draw::Segment& s, double big, int tile, int c, double (&u)[draw::kDrawPerLane]) {
  const long long start = (long long)tile * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  const int* order = a.order_inj + (long long)c * s.n;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    u[q] = 0.0;
    if (start + q < s.n) {
      const double v = draw::live_log_weight(s, order[start + q], a.d.log_const);
      if (v > -__builtin_inf()) u[q] = exp(v - big);
    }
  }
}

__global__ __launch_bounds__(kBlock) void rank_tile_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = (int)blockIdx.x, c = (int)blockIdx.y;
  const draw::Segment s = draw::segment_of(a.d, a.d.n_ev);
  double u[draw::kDrawPerLane], run = 0.0, total;
  gather_tile(a, s, a.d.seg_max[a.d.n_ev], tile, c, u);
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) run += u[q];
  (void)draw::block_inclusive_scan(run, lds, &total);
  if (threadIdx.x == 0) a.tile_sum[(long long)c * a.d.n_inj_tiles + tile] = total;
}

__global__ __launch_bounds__(kBlock) void rank_merge_kernel(const Args a) {
  if (threadIdx.x != 0) return;  // (no barrier below)
  const long long at = (long long)blockIdx.x * a.d.n_inj_tiles;
  double off = 0.0;
#pragma unroll 8
  for (int t = 0; t < a.d.n_inj_tiles; ++t) {
    a.tile_off[at + t] = off;
    off += a.tile_sum[at + t];
  }
}

__global__ __launch_bounds__(kBlock) void rank_prefix_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = (int)blockIdx.x, c = (int)blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const draw::Segment s = draw::segment_of(a.d, a.d.n_ev);
  double u[draw::kDrawPerLane], run = 0.0;
  gather_tile(a, s, a.d.seg_max[a.d.n_ev], tile, c, u);
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
  const double off = a.tile_off[(long long)c * a.d.n_inj_tiles + tile];
  double* out = a.prefix + (long long)c * (s.n + 1);
  if (tile == 0 && threadIdx.x == 0) out[0] = 0.0;
  const long long start = (long long)tile * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double c_r = before;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    c_r += u[q];
    if (start + q < s.n) out[start + q + 1] = off + c_r;
  }
}

__global__ __launch_bounds__(kBlock) void pit_rank_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = (int)blockIdx.x, c = (int)blockIdx.y, seg = tile / a.d.tiles_per_event;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double big = a.d.seg_max[seg];
  const double* prefix = a.prefix + (long long)c * (a.d.n_inj + 1);
  const long long at = ((long long)c * a.d.n_ev + seg) * a.d.n_pe;
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double lt = 0.0, le = 0.0;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const long long j = start + q;
    if (j < s.n) {
      const double v = draw::live_log_weight(s, j, a.d.log_const);
      if (v > -__builtin_inf()) {  // (a dead injection segment leaves nothing in P to read: its pit is NaN whatever is summed here)
        const double w = exp(v - big);
        lt += draw::scaled(w, prefix[a.rank_lt[at + j]]);
        le += draw::scaled(w, prefix[a.rank_le[at + j]]);
      }
    }
  }
  lt = draw::block_reduce(lt, lds, draw::OpAdd());
  le = draw::block_reduce(le, lds, draw::OpAdd());
  if (threadIdx.x == 0) {
    double* out = a.partial + ((long long)tile * a.n_cols + c) * 2;
    out[0] = lt;
    out[1] = le;
  }
}

__global__ __launch_bounds__(kBlock) void pit_rank_merge_kernel(const Args a) {
  if (threadIdx.x != 0) return;  // (no barrier below)
  const int seg = (int)blockIdx.x, c = (int)blockIdx.y, n_ev = a.d.n_ev;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total = s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool seg_live = live_total(total);
  if (c == 0) a.dead[seg] = seg_live ? 0 : 1;
  if (seg == n_ev) return;
  const double t_c = a.prefix[(long long)c * (a.d.n_inj + 1) + a.d.n_inj];
  // the injection segment's liveness is that of its S, as every other entry's; T_c is the same sum in another order
  const bool inj_live = a.d.n_inj_tiles > 0 && live_total(a.d.tile_prefix[n_ev * a.d.tiles_per_event + a.d.n_inj_tiles - 1]) && live_total(t_c);
  double* out = a.pit + ((long long)seg * a.n_cols + c) * 2;
  if (!seg_live || !inj_live) {
    out[0] = out[1] = __builtin_nan("");
    return;
  }
  const double* p = a.partial + ((long long)s.first_tile * a.n_cols + c) * 2;
  const long long stride = (long long)a.n_cols * 2;
  double lt = 0.0, le = 0.0;
#pragma unroll 8
  for (int t = 0; t < s.n_tiles; ++t) {
    lt += p[(long long)t * stride];
    le += p[(long long)t * stride + 1];
  }
  out[0] = lt / total / t_c;
  out[1] = le / total / t_c;
}

}  // namespace rank
}  // namespace gwi
