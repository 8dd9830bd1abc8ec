// gwi_quant.h -- marginal posterior weights of the samples and their weighted quantiles and moments: the credible intervals of the
// population-informed posterior of every event and of the predicted detected distribution, marginalised over hyper-parameter
// points (include/gwi_engine.h: gwi_marginal_weights_add, gwi_weighted_quantiles; the NumPy statement is gwinferno_amd/draws.py:
// marginal_weights_reference, weighted_quantiles_reference).
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's.  For one hyper-parameter point draw_tile_kernel and
// draw_merge_kernel (unchanged) give the segment maximum M and the tiles' inclusive mass prefix, whose last entry is the segment
// total S = sum_i w_i with w_i = exp(lw_i - M) (0 for a masked or non-finite sample) -- exactly the quantities of gwi_draw_indices
// and gwi_weighted_histograms.  One more launch follows per point:
//
//   marg_add_kernel      one lane per kDrawPerLane consecutive samples, tiles numbered as in DrawArgs: W_i += w_i / S on the running
//                        double per sample in HBM.  A segment whose S is 0 or not finite adds nothing; the lane of its first sample
//                        increments dead[segment], and otherwise adds the point's weight onto vsum[segment] and its square onto
//                        vsum2[segment]
//
// A point may carry a linear weight v in [0, 1] per segment (gwi_marginal_weights_add_weighted; marg_add_kernel<true>): the quotient
// w_i / S is formed as without it and then multiplied by v, in a product of its own that is not fused into the sum, so v = 1 gives the
// bits of the unweighted launch.  A point whose v is 0 touches nothing of its segment, dead[segment] included.  The unweighted launch
// counts v = 1: after unweighted points alone vsum[segment] is n_points - dead[segment].
//
// W_i = sum_k v_k w_{k,i} / S_k is the marginal posterior weight of sample i.  It does not depend on any quantile column and is not
// reset when the draw mask changes: a mask applies to the points added while it is set.
//
// A quantile column c supplies values x and, per segment, an int32 permutation of the segment's sample indices along which the
// values do not decrease (the library does not sort).  With C_r the inclusive prefix of W along that order and C_last the last
// prefix, the quantile of level p in [0, 1] (rule "inverted CDF") is the sample at the smallest rank r with C_r >= p C_last and
// W > 0 at that rank; the last rank with weight when rounding runs past the end; -1 when nothing has weight.  p = 0 is the smallest
// value with weight, p = 1 the largest.  The moments are m1 = sum W_i x_i and m2 = sum W_i x_i^2 along the same order.  Three
// launches per query:
//
//   quant_tile_kernel    one workgroup per (tile of kDrawTile ranks, column): W and x gathered through the order; the tile's sums of
//                        W, W x and W x^2 (four consecutive ranks per lane in rank order, then block_inclusive_scan's total)
//   quant_merge_kernel   one workgroup per (segment, column): the inclusive prefix of the tiles' sums of W in tile order -- its last
//                        entry is C_last -- and the two moments (the first half of the contract's select step: nothing here depends
//                        on the levels)
//   quant_select_kernel  one workgroup per (segment, column): for each level the first tile with weight whose prefix reaches the
//                        target (a block-wide search that passes over tiles without weight, as draw_select_kernel's), then that
//                        tile's ranks are gathered and scanned again -- lane order, wave scan, LDS across the four waves -- and the
//                        first hit is found with a ballot
//
// Every sum has a fixed shape -- rank order inside a tile, then tile order, then, for W, the order of the points on one stream -- so
// the bits of W, of the indices and of the moments are a pure function of the arguments and of the order of the points.  No atomics,
// nothing depends on which workgroup arrives first, every store is a plain vector store; no scratch.  The parallel prefixes are not
// monotone to the last bit, so a hit also requires W > 0, and the level whose target is C_last itself (p = 1) takes the last rank
// with weight directly.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace quant {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxCols = 8;
constexpr int kMaxLevels = 32;
constexpr int kSums = 3;  // per (tile, column): sum W, sum W x, sum W x^2

struct MargArgs {
  draw::DrawArgs d;  // the segments, the masks, log_const, seg_max and tile_prefix of this point
  double* w_pe;      // [n_ev][n_pe] running sums over the points
  double* w_inj;     // [n_inj]
  int* dead;         // [n_ev + 1]
  double* vsum;      // [n_ev + 1] running sum of the points' weights over the live points (1 per point without weights)
  double* vsum2;     // [n_ev + 1] ... of their squares
  const double* v;   // [n_ev + 1] this point's weight per segment (marg_add_kernel<true>; not read otherwise)
};

struct Args {
  const double* w_pe;     // [n_ev][n_pe] the marginal weights
  const double* w_inj;    // [n_inj]
  const double* x_pe;     // [n_cols][n_ev][n_pe]
  const double* x_inj;    // [n_cols][n_inj]
  const int* order_pe;    // [n_cols][n_ev][n_pe] per (column, event) a permutation of 0 ... n_pe - 1
  const int* order_inj;   // [n_cols][n_inj]
  double* partial;        // [n_tiles][n_cols][kSums], tiles numbered as in DrawArgs
  double* prefix;         // [n_tiles][n_cols] inclusive prefix of the tiles' sums of W within their segment
  const double* levels;   // [n_levels]
  int* idx;               // [n_ev + 1][n_cols][n_levels]; segment n_ev = the injection set
  double* moments;        // [n_ev + 1][n_cols][2]
  double* mass;           // [n_ev + 1]: C_last (of column 0's order)
  long long n_pe, n_inj;
  int n_ev, tiles_per_event, n_inj_tiles, n_cols, n_levels;
  int first_tile, first_seg;  // the launches cover tiles / segments from here on (a set without columns is left out)
};

// one segment's marginal weights and column c's values and order
struct Column {
  const double* w;
  const double* x;
  const int* order;
  long long n;
  int first_tile, n_tiles;
};

__device__ inline Column column_of(const Args& a, int seg, int c) {
  if (seg < a.n_ev) {
    const long long at = ((long long)c * a.n_ev + seg) * a.n_pe;
    return Column{a.w_pe + (long long)seg * a.n_pe, a.x_pe + at, a.order_pe + at, a.n_pe, seg * a.tiles_per_event, a.tiles_per_event};
  }
  const long long at = (long long)c * a.n_inj;
  return Column{a.w_inj, a.x_inj + at, a.order_inj + at, a.n_inj, a.n_ev * a.tiles_per_event, a.n_inj_tiles};
}

template <bool kWeighted>
__global__ __launch_bounds__(kBlock) void marg_add_kernel(const MargArgs a) {
  const int tile = blockIdx.x, n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
  const draw::Segment s = draw::segment_of(a.d, seg);
  double pv = 1.0;
  if constexpr (kWeighted) {
    pv = a.v[seg];
    if (pv == 0.0) return;  // (the same for every thread of the workgroup)
  }
  const double total = a.d.tile_prefix[s.first_tile + s.n_tiles - 1];  // (n_tiles >= 1: this tile exists)
  const bool first_lane = tile == s.first_tile && threadIdx.x == 0;    // one lane per segment and point
  if (!(total > 0.0 && total < __builtin_inf())) {
    if (first_lane) a.dead[seg] += 1;
    return;
  }
  if (first_lane) {
    a.vsum[seg] += pv;
    a.vsum2[seg] += pv * pv;
  }
  const double big = a.d.seg_max[seg];
  double* w = seg < a.d.n_ev ? a.w_pe + (long long)seg * a.d.n_pe : a.w_inj;
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const long long j = start + q;
    if (j < s.n) {
      const double v = draw::live_log_weight(s, j, a.d.log_const);
      if (v > -__builtin_inf()) {  // (a sample without weight would add +0.0)
        if constexpr (kWeighted) w[j] += draw::scaled(pv, exp(v - big) / total);
        else w[j] += exp(v - big) / total;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void quant_tile_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int tile = a.first_tile + (int)blockIdx.x, c = (int)blockIdx.y, n_pe_tiles = a.n_ev * a.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.tiles_per_event : a.n_ev;
  const Column col = column_of(a, seg, c);
  const long long start = (long long)(tile - col.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const long long r = start + q;
    if (r < col.n) {
      const int j = col.order[r];
      const double w = col.w[j], x = col.x[j], wx = w * x;
      s0 += w;
      s1 += wx;
      s2 += wx * x;
    }
  }
  double t0, t1, t2;
  (void)draw::block_inclusive_scan(s0, lds, &t0);
  (void)draw::block_inclusive_scan(s1, lds, &t1);
  (void)draw::block_inclusive_scan(s2, lds, &t2);
  if (threadIdx.x == 0) {
    double* out = a.partial + ((long long)tile * a.n_cols + c) * kSums;
    out[0] = t0;
    out[1] = t1;
    out[2] = t2;
  }
}

__global__ __launch_bounds__(kBlock) void quant_merge_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  const int seg = a.first_seg + (int)blockIdx.x, c = (int)blockIdx.y;
  const Column col = column_of(a, seg, c);
  double carry = 0.0, m1 = 0.0, m2 = 0.0;
  for (int base = 0; base < col.n_tiles; base += kBlock) {  // (the trip count is the same for every thread)
    const int t = base + (int)threadIdx.x;
    const double* p = a.partial + ((long long)(col.first_tile + t) * a.n_cols + c) * kSums;
    const double v0 = t < col.n_tiles ? p[0] : 0.0, v1 = t < col.n_tiles ? p[1] : 0.0, v2 = t < col.n_tiles ? p[2] : 0.0;
    double t0, t1, t2;
    const double incl = draw::block_inclusive_scan(v0, lds, &t0);
    (void)draw::block_inclusive_scan(v1, lds, &t1);
    (void)draw::block_inclusive_scan(v2, lds, &t2);
    if (t < col.n_tiles) a.prefix[(long long)(col.first_tile + t) * a.n_cols + c] = carry + incl;
    carry += t0;
    m1 += t1;
    m2 += t2;
  }
  if (threadIdx.x == 0) {
    double* out = a.moments + ((long long)seg * a.n_cols + c) * 2;
    out[0] = m1;
    out[1] = m2;
  }
}

__global__ __launch_bounds__(kBlock) void quant_select_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  __shared__ int ldi[kBlock / 64];
  const int seg = a.first_seg + (int)blockIdx.x, c = (int)blockIdx.y;
  const Column col = column_of(a, seg, c);
  const long long stride = a.n_cols;
  const double* prefix = a.prefix + (long long)col.first_tile * stride + c;                // tile t: prefix[t * stride]
  const double* mass = a.partial + ((long long)col.first_tile * stride + c) * kSums;       // tile t: mass[t * stride * kSums]
  const double c_last = col.n_tiles > 0 ? prefix[(long long)(col.n_tiles - 1) * stride] : 0.0;
  int* out = a.idx + ((long long)seg * a.n_cols + c) * a.n_levels;
  if (c == 0 && threadIdx.x == 0) a.mass[seg] = c_last;
  for (int q = 0; q < a.n_levels; ++q) {
    if (!(c_last > 0.0)) {  // (the same for every thread of the workgroup, like every branch around a barrier below)
      if (threadIdx.x == 0) out[q] = -1;
      continue;
    }
    const double target = a.levels[q] * c_last;
    const bool top = !(target < c_last);  // p = 1: the last rank with weight
    // the tile: the first one with weight whose prefix reaches the target, else the last one with weight
    int first = draw::kDrawNone, last = -1;
    for (int t = threadIdx.x; t < col.n_tiles; t += kBlock)
      if (mass[(long long)t * stride * kSums] > 0.0) {
        last = t;
        if (!top && first == draw::kDrawNone && prefix[(long long)t * stride] >= target) first = t;
      }
    first = draw::block_reduce(first, ldi, draw::OpMin());
    last = draw::block_reduce(last, ldi, draw::OpMax());
    const int tile = first != draw::kDrawNone ? first : last;  // c_last > 0: some tile has weight
    const double rest = target - (tile > 0 ? prefix[(long long)(tile - 1) * stride] : 0.0);
    // ... and the rank inside it
    const int j0 = (int)threadIdx.x * draw::kDrawPerLane;
    const long long start = (long long)tile * kTile + j0;
    double w[draw::kDrawPerLane], run = 0.0;
#pragma unroll
    for (int i = 0; i < draw::kDrawPerLane; ++i) {
      w[i] = start + i < col.n ? col.w[col.order[start + i]] : 0.0;
      run += w[i];
    }
    double total;
    const double before = draw::block_inclusive_scan(run, lds, &total) - run;
    int hit = draw::kDrawNone, live = -1;
    double c_r = before;
#pragma unroll
    for (int i = 0; i < draw::kDrawPerLane; ++i) {
      c_r += w[i];
      if (w[i] > 0.0) {
        live = j0 + i;
        if (!top && hit == draw::kDrawNone && c_r >= rest) hit = j0 + i;
      }
    }
    // the first lane of a wave with a hit holds the wave's smallest rank: lanes hold ascending ranks
    const unsigned long long any = __ballot(hit != draw::kDrawNone);
    const int wave_hit = any ? __shfl(hit, __ffsll((long long)any) - 1) : draw::kDrawNone;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ldi[threadIdx.x >> 6] = wave_hit;
    __syncthreads();
    int sel = draw::kDrawNone;
    for (int wv = kBlock / 64 - 1; wv >= 0; --wv)
      if (ldi[wv] != draw::kDrawNone) sel = ldi[wv];
    if (sel == draw::kDrawNone) sel = draw::block_reduce(live, ldi, draw::OpMax());  // rounding ran past the tile's end, or p = 1 (sel is uniform: so is the branch)
    if (threadIdx.x == 0) out[q] = sel >= 0 ? col.order[(long long)tile * kTile + sel] : -1;
  }
}

}  // namespace quant
}  // namespace gwi
