// gwi_hist.h -- weighted histograms of the per-sample weights the log-weight role of a scan chain leaves in HBM: the
// population-informed posterior of every event and the predicted detected distribution of the injection set, summed over
// hyper-parameter points (include/gwi_engine.h: gwi_weighted_histograms; the NumPy statement is gwinferno_amd/draws.py:
// weighted_histograms_reference; the deterministic counterpart of the observed-versus-predicted check in the reference's
// posterior-predictive branch, pipeline/analysis.py:321-355).
//
// Segments, tiles and live_log_weight() are gwi_draw.h's.  For one hyper-parameter point draw_tile_kernel and draw_merge_kernel
// give the segment maximum M and the tiles' inclusive mass prefix, whose last entry is the segment total S = sum_i exp(lw_i - M).
// Two more launches follow:
//
//   hist_tile_kernel    one workgroup per tile of kDrawTile samples: w_i = exp(lw_i - M) (0 for a masked or non-finite sample) once
//                       per tile into LDS beside the tile's uint16 bin codes of all C columns; then thread (c, b) adds the w_i of the
//                       samples whose code in column c is b, in sample order, and stores P[tile][c][b]
//   hist_merge_kernel   one workgroup per (segment, column): thread b adds P[tile][c][b] over the segment's tiles in tile order,
//                       divides by S and adds the quotient onto the running sum H[segment][c][b] in HBM; a segment whose S is 0 or
//                       not finite adds nothing and is counted in n_dead[segment] (by the workgroup of column 0 alone)
//
// A point may carry a linear weight v in [0, 1] per segment (gwi_weighted_histograms_weighted; hist_merge_kernel<true>): the quotient
// is formed as without it and then multiplied by v, in a product of its own that is not fused into the sum, so v = 1 gives the bits
// of the unweighted launch; the lane that counts n_dead adds v onto vsum[segment] for a live segment instead.  A point whose v is 0
// touches nothing of its segment, n_dead[segment] included.  The tile launch does not depend on v.
//
// Every sum has a fixed shape -- sample order within a tile and bin, then tile order, then the order of the points (the launches
// of one point follow those of the previous one on one stream) -- so the bits of H are a pure function of the inputs.  No atomics,
// nothing depends on which workgroup arrives first, every store is a plain vector store; no scratch.  Adding the +0.0 of a sample
// in another bin leaves a non-negative partial sum as it is, so the tile loop has no branch.  A code of kOutside (or any code that
// is no bin) is in no bin but still counts in S: H sums to at most 1 over a column's bins, the deficit is the weight outside.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace hist {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxCols = 8;
constexpr int kMaxBins = kBlock;            // thread b of the merge workgroup owns bin b
constexpr unsigned short kOutside = 0xFFFF;  // "outside every bin"

struct Args {
  draw::DrawArgs d;               // the segments, the masks, log_const, seg_max and tile_prefix of this point
  const unsigned short* bins_pe;  // [n_cols][n_ev][n_pe]
  const unsigned short* bins_inj; // [n_cols][n_inj]
  double* partial;                // [n_tiles][n_cols][n_bins], tiles numbered as in DrawArgs
  double* hist;                   // [n_ev + 1][n_cols][n_bins] running sums over the points; segment n_ev = the injection set
  int* n_dead;                    // [n_ev + 1]
  const double* v;                // [n_ev + 1] this point's weight per segment (hist_merge_kernel<true>; not read otherwise)
  double* vsum;                   // [n_ev + 1] running sum of the weights over the live points (hist_merge_kernel<true>)
  int n_cols, n_bins;
  int first_tile, first_seg;      // the launch covers tiles / segments from here on (a set without bins is left out)
};

__global__ __launch_bounds__(kBlock) void hist_tile_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) double w_lds[kTile];
  __shared__ __attribute__((aligned(16))) unsigned short code_lds[kMaxCols][kTile];
  const int tile = a.first_tile + (int)blockIdx.x, n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double big = a.d.seg_max[seg];
  const long long tile_start = (long long)(tile - s.first_tile) * kTile;
  const int count = (int)(s.n - tile_start < kTile ? s.n - tile_start : kTile);  // (>= 1: the tile exists)
  const int j0 = (int)threadIdx.x * draw::kDrawPerLane;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const int j = j0 + q;
    double w = 0.0;
    if (j < count) {
      const double v = draw::live_log_weight(s, tile_start + j, a.d.log_const);
      w = v > -__builtin_inf() ? exp(v - big) : 0.0;
    }
    w_lds[j] = w;
  }
  for (int c = 0; c < a.n_cols; ++c) {
    const unsigned short* codes = seg < a.d.n_ev ? a.bins_pe + ((long long)c * a.d.n_ev + seg) * a.d.n_pe + tile_start : a.bins_inj + (long long)c * a.d.n_inj + tile_start;
#pragma unroll
    for (int q = 0; q < draw::kDrawPerLane; ++q) code_lds[c][j0 + q] = j0 + q < count ? codes[j0 + q] : kOutside;
  }
  __syncthreads();
  const int n_items = a.n_cols * a.n_bins, end = (count + 3) & ~3;  // (the entries past count hold weight 0 and kOutside)
  double* out = a.partial + (long long)tile * n_items;
  for (int item = threadIdx.x; item < n_items; item += kBlock) {  // (no barrier in the loop)
    const int c = item / a.n_bins;
    const unsigned b = (unsigned)(item - c * a.n_bins);
    const unsigned short* codes = code_lds[c];
    double acc = 0.0;
    for (int i = 0; i < end; i += 4) {
      const uint2 k = *reinterpret_cast<const uint2*>(codes + i);
      const double2 w01 = *reinterpret_cast<const double2*>(w_lds + i), w23 = *reinterpret_cast<const double2*>(w_lds + i + 2);
      acc += (k.x & 0xFFFFu) == b ? w01.x : 0.0;
      acc += (k.x >> 16) == b ? w01.y : 0.0;
      acc += (k.y & 0xFFFFu) == b ? w23.x : 0.0;
      acc += (k.y >> 16) == b ? w23.y : 0.0;
    }
    out[item] = acc;
  }
}

template <bool kWeighted>
__global__ __launch_bounds__(kBlock) void hist_merge_kernel(const Args a) {
  const int seg = a.first_seg + (int)blockIdx.x, c = (int)blockIdx.y, b = (int)threadIdx.x;
  double pv = 1.0;
  if constexpr (kWeighted) {
    pv = a.v[seg];
    if (pv == 0.0) return;  // (the same for every thread of the workgroup)
  }
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total = s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool live = total > 0.0 && total < __builtin_inf();
  if (!live) {
    if (c == 0 && b == 0) a.n_dead[seg] += 1;
    return;
  }
  if constexpr (kWeighted)
    if (c == 0 && b == 0) a.vsum[seg] += pv;
  if (b >= a.n_bins) return;
  const long long stride = (long long)a.n_cols * a.n_bins;
  const double* p = a.partial + (long long)s.first_tile * stride + (long long)c * a.n_bins + b;
  double sum = 0.0;
#pragma unroll 8
  for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * stride];
  double* h = a.hist + ((long long)seg * a.n_cols + c) * a.n_bins + b;
  if constexpr (kWeighted) *h += draw::scaled(pv, sum / total);
  else *h += sum / total;
}

}  // namespace hist
}  // namespace gwi
