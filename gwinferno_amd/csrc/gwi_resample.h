// gwi_resample.h -- many seeded draws from the injection set's weights, with the sums the reference's resample_injections needs
// (include/gwi_engine.h: gwi_resample_injections; preprocess/selection.py:143-156; the NumPy statement is
// gwinferno_amd/draws.py: resample_indices_reference).
//
// The log-weight role of the scan chain leaves lw_j in HBM and draw_tile_kernel / draw_merge_kernel (gwi_draw.h) reduce the
// injection segment to M, every tile's mass and the tiles' inclusive prefix.  With w_j = exp(lw_j + log_const - M) (0 for a
// masked, non-finite or out-of-range sample: live_log_weight's rule) three more launches follow:
//
//   resample_prefix_kernel  one workgroup per tile of kDrawTile samples: the in-tile inclusive prefix in draw_select_kernel's
//                           shape (four consecutive samples per lane added in order, then the block scan) into HBM, 8 B per
//                           injection; the tile's sum of w^2 and its number of samples with weight through the block reduction
//   resample_stats_kernel   one workgroup: Q = the sum over tiles of sum w^2 (chunks of 256 with a carry, draw_merge_kernel's
//                           shape), C_last, the last tile with mass, the number of samples with weight, M -- the few doubles the
//                           host reads before it sizes the draw: n_eff = C_last^2 / Q
//   resample_select_kernel  lane = draw, grid-stride.  Draw d of the launch has stream index first_index + d and takes ONE
//                           Philox4x32-10 block -- counter (index low, index high, 0, kTag), key = the seed's halves; u = words 0, 1.
//                           A binary search over the tile prefix finds a tile whose prefix exceeds u C_last while its
//                           predecessor's does not; a tile without mass is passed over for the next one with mass, past the end
//                           the last tile with mass is taken.  Inside the tile the stored prefix is searched the same way against
//                           the rest of the target: the first sample with w_j > 0 from there on, else the tile's last sample with
//                           weight (the parallel prefixes are not monotone to the last bit: gwi_popdraw.h's two rules).  The lane
//                           writes the index and lw_j + log_const of the drawn sample; -1 and NaN when nothing has weight.
//
// Every sum has a fixed shape, so the prefixes -- and with them every draw -- are the same bits on every call.  Plain vector loads
// and stores, no atomics, no scratch, no LDS staging of the prefixes (they are read from HBM / L2).  Every loop is bounded by the
// number of tiles or by kDrawTile.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"
#include "gwi_spinprior.h"

namespace gwi {
namespace resample {

constexpr int kBlock = draw::kDrawBlock;  // the block scan and reduction of gwi_draw.h are written for it
constexpr int kTile = draw::kDrawTile;
constexpr unsigned kTag = 0x52534D50u;    // counter word 3 ("RSMP"); population draws use 0x504F5044, the chi_p kernel < 2^17
constexpr int kStats = 5;                 // doubles of the stats record, in this order:
enum { kStatQ = 0, kStatCLast = 1, kStatLastTile = 2, kStatLive = 3, kStatMax = 4 };

struct Args {
  const double* lw;            // [n] log-weights without the sample-independent constant
  const unsigned char* mask;   // [n] or nullptr: every sample may be drawn
  const double* seg_max;       // [1] M of the segment (draw_merge_kernel)
  const double* tile_mass;     // [n_tiles]
  const double* tile_prefix;   // [n_tiles]
  double* sample_prefix;       // [n] inclusive prefix of w inside each tile
  double* tile_sq;             // [n_tiles] sum of w^2
  int* tile_live;              // [n_tiles] samples with w > 0
  double* stats;               // [kStats]
  int* idx;                    // [n_draws of this launch]
  double* lw_sel;              // [n_draws of this launch]
  double log_const;
  unsigned long long seed, first_index;  // first_index: the stream index of this launch's draw 0
  long long n, n_draws;
  int n_tiles, n_lanes;        // n_lanes: threads of the select launch (the grid stride)
};

// w_j of sample j
__device__ inline double weight_of(const Args& a, long long j, double big) {
  const draw::Segment s{a.lw, a.mask, a.n, 0, a.n_tiles};
  const double v = draw::live_log_weight(s, j, a.log_const);
  return v > -__builtin_inf() ? exp(v - big) : 0.0;
}

__global__ __launch_bounds__(kBlock) void resample_prefix_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  __shared__ int ldi[kBlock / 64];
  const double big = a.seg_max[0];
  const long long start = (long long)blockIdx.x * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
  double w[draw::kDrawPerLane], run = 0.0, sq = 0.0;
  int live = 0;
#pragma unroll
  for (int c = 0; c < draw::kDrawPerLane; ++c) {
    w[c] = start + c < a.n ? weight_of(a, start + c, big) : 0.0;
    run += w[c];
    sq += w[c] * w[c];
    live += w[c] > 0.0 ? 1 : 0;
  }
  double total;
  double c_j = draw::block_inclusive_scan(run, lds, &total) - run;
#pragma unroll
  for (int c = 0; c < draw::kDrawPerLane; ++c) {
    c_j += w[c];
    if (start + c < a.n) a.sample_prefix[start + c] = c_j;
  }
  sq = draw::block_reduce(sq, lds, draw::OpAdd());
  live = draw::block_reduce(live, ldi, draw::OpAdd());
  if (threadIdx.x == 0) {
    a.tile_sq[blockIdx.x] = sq;
    a.tile_live[blockIdx.x] = live;
  }
}

__global__ __launch_bounds__(kBlock) void resample_stats_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  __shared__ int ldi[kBlock / 64];
  double carry = 0.0, n_live = 0.0;  // (a count below 2^31: exact in a double in any order)
  int last = -1;
  for (int base = 0; base < a.n_tiles; base += kBlock) {  // (the trip count is the same for every thread)
    const int t = base + (int)threadIdx.x;
    const bool in = t < a.n_tiles;
    if (in && a.tile_mass[t] > 0.0) last = t;
    if (in) n_live += (double)a.tile_live[t];
    double total;
    (void)draw::block_inclusive_scan(in ? a.tile_sq[t] : 0.0, lds, &total);
    carry += total;
  }
  last = draw::block_reduce(last, ldi, draw::OpMax());
  n_live = draw::block_reduce(n_live, lds, draw::OpAdd());
  if (threadIdx.x == 0) {
    a.stats[kStatQ] = carry;
    a.stats[kStatCLast] = a.n_tiles > 0 ? a.tile_prefix[a.n_tiles - 1] : 0.0;
    a.stats[kStatLastTile] = (double)last;
    a.stats[kStatLive] = n_live;
    a.stats[kStatMax] = a.seg_max[0];
  }
}

__global__ __launch_bounds__(kBlock) void resample_select_kernel(const Args a) {
#pragma clang fp contract(off)
  const double big = a.stats[kStatMax], c_last = a.stats[kStatCLast];
  const int last_tile = (int)a.stats[kStatLastTile];
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
  for (long long d = (long long)blockIdx.x * kBlock + threadIdx.x; d < a.n_draws; d += a.n_lanes) {  // (no barrier in the loop)
    int sel = -1;
    long long at = -1;
    if (last_tile >= 0 && c_last > 0.0) {
      const unsigned long long index = a.first_index + (unsigned long long)d;
      const spinprior::U4 r = spinprior::philox4x32_10(spinprior::U4{(unsigned)index, (unsigned)(index >> 32), 0u, kTag}, k0, k1);
      const double target = spinprior::uniform53(r.x, r.y) * c_last;
      // a tile whose prefix exceeds the target while its predecessor's does not
      int lo = 0, hi = a.n_tiles;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.tile_prefix[mid] > target) hi = mid;
        else lo = mid + 1;
      }
      int tile = lo;
      while (tile < a.n_tiles && !(a.tile_mass[tile] > 0.0)) ++tile;  // never a tile without mass
      if (tile >= a.n_tiles) tile = last_tile;                         // past the end: the last tile with mass
      const double rest = target - (tile > 0 ? a.tile_prefix[tile - 1] : 0.0);
      // ... and the sample inside it, by the same two rules
      const long long first = (long long)tile * kTile;
      const int count = (int)(a.n - first < kTile ? a.n - first : kTile);  // (>= 1: the tile exists)
      const double* prefix = a.sample_prefix + first;
      lo = 0, hi = count;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] > rest) hi = mid;
        else lo = mid + 1;
      }
      sel = lo;
      while (sel < count && !(weight_of(a, first + sel, big) > 0.0)) ++sel;
      if (sel >= count) {  // rounding ran past the tile's end: its last sample with weight
        sel = count - 1;
        while (sel >= 0 && !(weight_of(a, first + sel, big) > 0.0)) --sel;
      }
      if (sel >= 0) at = first + sel;
    }
    a.idx[d] = (int)at;
    a.lw_sel[d] = at >= 0 ? a.lw[at] + a.log_const : __builtin_nan("");
  }
}

}  // namespace resample
}  // namespace gwi
