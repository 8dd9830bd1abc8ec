// gwi_cdf.h -- per-point cumulative distributions of the binned weights of gwi_hist.h, and what a catalog-level predictive check
// needs of them: the CDF of the predicted detected distribution, the mean of the events' CDFs and the log CDFs of the catalog's
// largest and smallest value, for ONE hyper-parameter point at a time (include/gwi_engine.h: gwi_point_cdfs; the NumPy statement is
// gwinferno_amd/draws.py: point_cdfs_reference; the contract is DESIGN 8g).  A percentile band over the points and a product over the
// events are not linear in the per-point distributions, so they cannot be rebuilt from the sums over points gwi_hist.h returns.
//
// The bins are cumulative codes (draws.py: cdf_codes): code j < G means g_{j-1} < x <= g_j, anything above the grid or NaN is kOutside
// and counts in S alone, so the running sum of a column's bins up to j is exactly the weight share with x <= g_j.
//
// Segments, tiles, M, S and P[tile][c][b] are gwi_draw.h's and gwi_hist.h's: per point the launches follow the log-weight pass,
// draw_tile_kernel, draw_merge_kernel and hist_tile_kernel, all unchanged.  Two launches replace hist_merge_kernel:
//
//   cdf_segment_kernel   one workgroup per (segment, column): thread b adds P[tile][c][b] over the segment's tiles in tile order and
//                        divides by S -- hist_merge_kernel<false>'s expression, so its bits -- writes the quotient to LDS, and after
//                        the workgroup's one barrier adds entries 0 ... b from LDS left to right and stores F[segment][c][b].  The
//                        prefix is SEQUENTIAL on purpose (at most 256 LDS reads per thread, every one a broadcast: the lanes of a
//                        wave that are still in the loop read the same double): those are the bits of np.cumsum.  No tree scan.
//                        The workgroup of column 0 stores the segment's flag, 1 where S is 0 or not finite (hist_merge_kernel's rule);
//                        such a segment stores nothing else
//   cdf_catalog_kernel   one workgroup per column: thread b walks the events in order, skips the flagged ones and adds F, log F and
//                        log1p(-min(F, 1)); it stores the point's four slots [4][n_cols][n_bins] -- F of the injection segment; the
//                        sum of F over one division by the number of live events; the two sums of logarithms -- into the point's row
//                        of the staging buffer, and thread 0 of column 0 stores (live events, injection segment live)
//
// Every sum has a fixed shape -- tile order, bin order, event order -- there are no atomics, nothing depends on which workgroup arrives
// first, every store is a plain vector store; no scratch.  log 0 = -inf stays (an event without weight at or below g_b makes the
// catalog's maximum certainly larger).  A slot without its set's bins, slot 0 of a dead injection segment and slot 1 without a live
// event are NaN; the sums of slots 2 and 3 over no live event are 0.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_hist.h"

namespace gwi {
namespace cdf {

constexpr int kBlock = hist::kBlock;
constexpr int kSlots = 4;        // cdf_det, cdf_obs, log_all_below, log_all_above

struct Args {
  hist::Args h;     // the segments, S, the tiles' partial histograms, n_cols, n_bins, first_seg of this point (hist and n_dead are not touched)
  double* cdf;      // [n_ev + 1][n_cols][n_bins] F of this point
  int* seg_dead;    // [n_ev + 1] 1: the segment has no weight at this point
  double* out;      // [kSlots][n_cols][n_bins] the point's row of the staging buffer
  int* live;        // [2] the point's (live events, injection segment live)
  int with_pe, with_inj;  // the sets that have bins
};

__global__ __launch_bounds__(kBlock) void cdf_segment_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) double q_lds[hist::kMaxBins];
  const int seg = a.h.first_seg + (int)blockIdx.x, c = (int)blockIdx.y, b = (int)threadIdx.x;
  const draw::Segment s = draw::segment_of(a.h.d, seg);
  const double total = s.n_tiles > 0 ? a.h.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool live = total > 0.0 && total < __builtin_inf();
  if (c == 0 && b == 0) a.seg_dead[seg] = live ? 0 : 1;
  if (!live) return;  // (the same for every thread of the workgroup)
  double q = 0.0;
  if (b < a.h.n_bins) {
    const long long stride = (long long)a.h.n_cols * a.h.n_bins;
    const double* p = a.h.partial + (long long)s.first_tile * stride + (long long)c * a.h.n_bins + b;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * stride];
    q = sum / total;
  }
  q_lds[b] = q;
  __syncthreads();
  if (b >= a.h.n_bins) return;
  double f = q_lds[0];
  for (int i = 1; i <= b; ++i) f += q_lds[i];
  a.cdf[((long long)seg * a.h.n_cols + c) * a.h.n_bins + b] = f;
}

__global__ __launch_bounds__(kBlock) void cdf_catalog_kernel(const Args a) {
  const int c = (int)blockIdx.x, b = (int)threadIdx.x, n_ev = a.h.d.n_ev, n_bins = a.h.n_bins;
  const long long per_seg = (long long)a.h.n_cols * n_bins, at = (long long)c * n_bins + b;
  const double nan = __builtin_nan("");
  int n_live = 0;
  double sum_f = 0.0, sum_below = 0.0, sum_above = 0.0;
  if (a.with_pe)
    for (int e = 0; e < n_ev; ++e) {
      if (a.seg_dead[e]) continue;  // (the same for every thread)
      ++n_live;
      if (b < n_bins) {
        const double f = a.cdf[e * per_seg + at];
        sum_f += f;
        sum_below += log(f);
        sum_above += log1p(-(f < 1.0 ? f : 1.0));
      }
    }
  const bool inj_live = a.with_inj && !a.seg_dead[n_ev];
  if (c == 0 && b == 0) {
    a.live[0] = n_live;
    a.live[1] = inj_live ? 1 : 0;
  }
  if (b >= n_bins) return;
  a.out[at] = inj_live ? a.cdf[n_ev * per_seg + at] : nan;
  a.out[per_seg + at] = n_live > 0 ? sum_f / (double)n_live : nan;
  a.out[2 * per_seg + at] = a.with_pe ? sum_below : nan;
  a.out[3 * per_seg + at] = a.with_pe ? sum_above : nan;
}

}  // namespace cdf
}  // namespace gwi
