// gwi_pit.h -- per-event calibration: for ONE hyper-parameter point at a time, a rigorous bracket of every event's probability integral
// transform under the predicted detected distribution, PIT = sum_i (w_i / S_e) F_det(x_i) (include/gwi_engine.h: gwi_point_pits; the
// NumPy statement is gwinferno_amd/draws.py: point_pits_reference, pit_bracket; the contract is DESIGN 8h).  The PIT is a product of two
// per-point objects -- the event's weights and the injection set's CDF -- so neither the sums over points of gwi_hist.h nor the catalog
// aggregates of gwi_cdf.h can give it; with leave-one-out weights on the k axis it is needed per (point, event).
//
// The bins are gwi_cdf.h's cumulative codes: code j < G means g_{j-1} < x <= g_j, so F_det of such a sample lies in [D[j-1], D[j]]
// (D[-1] := 0) with D the injection segment's CDF at the grid points, and F_det of a sample outside the grid in [D[G-1], 1].
//
// Per point the launches of gwi_point_cdfs run unchanged up to and including cdf_segment_kernel, which leaves F[segment][c][b] and the
// segments' flags.  One launch follows:
//
//   pit_kernel   one workgroup per (segment, column).  For an event: thread b forms q[b], the event's normalised bin, by
//                cdf_segment_kernel's expression (the tile-order sum over S: its bits, those of gwi_weighted_histograms for the single
//                point) and writes it to LDS beside D[b], read from the injection row of F; thread 0 adds o = max(0, 1 - F_e[G-1]), the
//                share outside the grid, as entry G.  After the workgroup's one barrier lanes 0 and 1 walk the G entries in order,
//                         lane 0   pit_lo = q[1] D[0] + q[2] D[1] + ... + q[G-1] D[G-2] + o D[G-1]
//                         lane 1   pit_hi = q[0] D[0] + q[1] D[1] + ... + q[G-1] D[G-1] + o
//                every product and every sum rounded on its own (no contraction), strictly left to right from 0.0, the outside term
//                last: the bits of a plain Python loop.  The walk is SEQUENTIAL on purpose, as the prefix of cdf_segment_kernel: at most
//                256 dependent steps fed by LDS reads two lanes wide.  A dead event or a dead injection segment gives NaN.  Thread 0 of
//                column 0 stores the event's flag.  For the injection segment (the last workgroup row): thread b copies D[b] (NaN if
//                the segment is dead) and thread 0 of column 0 stores its flag.
//
// No atomics, nothing depends on which workgroup arrives first, every store is a plain vector store; no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_cdf.h"

namespace gwi {
namespace pit {

constexpr int kBlock = cdf::kBlock;

struct Args {
  cdf::Args f;      // what cdf_segment_kernel saw and left: the tiles' partial histograms, S, F and the segments' flags of this point
  double* pit;      // [n_ev][n_cols][2] (lo, hi): the point's row of the staging buffer
  double* cdf_det;  // [n_cols][n_bins] F of the injection segment: the point's row of its staging buffer
  int* dead;        // [n_ev + 1] the point's row of the flags' staging buffer
};

// lane 0: the lower end, lane 1: the upper end of the bracket, from q[0 ... G] (entry G is o) and D[0 ... G-1]
__device__ inline double walk(const double* q, const double* d, int n_bins, int upper) {
#pragma clang fp contract(off)
  double acc = 0.0;
  const double* qs = q + (upper ? 0 : 1);
  for (int j = 0; j < n_bins; ++j) {
    const double term = qs[j] * d[j];
    acc = acc + term;
  }
  if (upper) acc = acc + q[n_bins];
  return acc;
}

__global__ __launch_bounds__(kBlock) void pit_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) double q_lds[hist::kMaxBins + 1];
  __shared__ __attribute__((aligned(16))) double d_lds[hist::kMaxBins];
  const hist::Args& h = a.f.h;
  const int seg = (int)blockIdx.x, c = (int)blockIdx.y, b = (int)threadIdx.x, n_ev = h.d.n_ev, n_bins = h.n_bins;
  const double nan = __builtin_nan("");
  const bool inj_dead = a.f.seg_dead[n_ev] != 0, seg_dead = a.f.seg_dead[seg] != 0;  // (the same for every thread of the workgroup)
  if (c == 0 && b == 0) a.dead[seg] = seg_dead ? 1 : 0;
  const double* d_row = a.f.cdf + ((long long)n_ev * h.n_cols + c) * n_bins;
  if (seg == n_ev) {
    if (b < n_bins) a.cdf_det[(long long)c * n_bins + b] = inj_dead ? nan : d_row[b];
    return;
  }
  double* out = a.pit + ((long long)seg * h.n_cols + c) * 2;
  if (seg_dead || inj_dead) {
    if (b < 2) out[b] = nan;
    return;
  }
  const draw::Segment s = draw::segment_of(h.d, seg);
  const double total = h.d.tile_prefix[s.first_tile + s.n_tiles - 1];  // (live: the segment has tiles)
  if (b < n_bins) {
    const long long stride = (long long)h.n_cols * n_bins;
    const double* p = h.partial + (long long)s.first_tile * stride + (long long)c * n_bins + b;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * stride];
    q_lds[b] = sum / total;
    d_lds[b] = d_row[b];
  }
  if (b == 0) {
    const double above = 1.0 - a.f.cdf[((long long)seg * h.n_cols + c) * n_bins + n_bins - 1];
    q_lds[n_bins] = above > 0.0 ? above : 0.0;
  }
  __syncthreads();
  if (b < 2) out[b] = walk(q_lds, d_lds, n_bins, b);
}

}  // namespace pit
}  // namespace gwi
