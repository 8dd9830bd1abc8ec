// gwi_hist2d.h -- joint (two-dimensional) weighted histograms per hyper-parameter point: for a pair (cx, cy) of the bin columns of
// gwi_set_histogram_bins the B x B table of every segment's weight shares, the observed catalog's table (the equal-weight mixture of
// the live events) and the table the injections predict for detected sources (include/gwi_engine.h: gwi_point_histograms2d; the NumPy
// statement is gwinferno_amd/draws.py: point_histograms2d_reference; the contract is DESIGN 8o).
//
// Segments, tiles and live_log_weight() are gwi_draw.h's; the codes and kOutside are gwi_hist.h's.  For one hyper-parameter point
// draw_tile_kernel and draw_merge_kernel give the segment maximum M and the tiles' inclusive mass prefix, whose last entry is the
// segment total S.  Three more launches follow PER PAIR, pair after pair on one stream, so that the partials of one pair are the
// whole workspace:
//
//   hist2d_tile_kernel    one workgroup per tile of kDrawTile samples: w_i = exp(lw_i - M) (0 for a masked or non-finite sample) once
//                         per tile into LDS, exactly hist_tile_kernel's staging, beside the joint code j = code_x B + code_y (kNoCell
//                         when either code is kOutside or no bin).  The B B cells live in LDS and cell j belongs to thread j mod 256
//                         alone: every thread walks the tile's codes in sample order (LDS broadcast reads, four codes per read) and adds
//                         w_i to the cells it owns.  Then it stores its cells: P[tile][cell]
//   hist2d_merge_kernel   one workgroup per (segment, block of 256 cells): a thread adds P[tile][cell] over the segment's tiles in tile
//                         order, divides by S and stores the share Q[segment][cell]; with running sums it also adds the share -- times the
//                         point's weight v, in a product of its own (draw::scaled) -- onto H[segment][pair][cell].  A segment whose S is 0 or
//                         not finite gets a NaN row of Q and seg_dead = 1, adds nothing and is counted in n_dead once per point (by the
//                         launch of the first pair)
//   hist2d_mix_kernel     one thread per cell: obs = (sum of Q[e][cell] over the live events e, in event order) / n_live and pred =
//                         Q[n_ev][cell] into the point's staged rows (NaN without a live event / with a dead injection set / for a set
//                         without bins); the launch of the first pair stores (n_live, injection set live)
//
// Q does not depend on v: a point's obs and pred rows are the same with and without point weights; v = 0 leaves H, n_dead and vsum of
// the segment alone.  Every sum has a fixed shape -- sample order within a tile and cell, then tile order, then event order for obs, then
// the order of the points for H -- so the bits are a pure function of the inputs.  No atomics, nothing depends on which workgroup
// arrives first, every store is a plain vector store; no scratch.  A pair (c, c) has the summation shape of hist_tile_kernel and
// hist_merge_kernel on its diagonal: the bits of gwi_weighted_histograms for column c at the point.
//
// LDS of the tile kernel: 8 KB of weights, 2 KB of joint codes (static) and 8 B B bytes of cells (dynamic; 32 KB at the cap B = 64):
// 42 KB at most, three workgroups per CU.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_hist.h"

namespace gwi {
namespace hist2d {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kMaxBins = 64;                 // per axis: 4 096 cells, 32 KB of doubles
constexpr int kMaxPairs = 8;
constexpr unsigned kNoCell = 0xFFFFu;        // joint code of a sample in no cell (>= kMaxBins kMaxBins)

struct Args {
  draw::DrawArgs d;               // the segments, the masks, log_const, seg_max and tile_prefix of this point
  const unsigned short* bins_pe;  // [n_cols][n_ev][n_pe]   (gwi_set_histogram_bins)
  const unsigned short* bins_inj; // [n_cols][n_inj]
  double* partial;                // [n_tiles][n_bins n_bins] of the current pair, tiles numbered as in DrawArgs
  double* share;                  // Q [n_ev + 1][n_bins n_bins] of the current pair
  int* seg_dead;                  // [n_ev + 1] of this point
  double* hist;                   // H [n_ev + 1][n_pairs][n_bins n_bins] running sums over the points, or nullptr
  int* n_dead;                    // [n_ev + 1] running counts, or nullptr
  const double* v;                // [n_ev + 1] this point's weight per segment, or nullptr (every weight 1)
  double* vsum;                   // [n_ev + 1] running sum of the weights over the live points, or nullptr
  double* obs;                    // [n_pairs][n_bins n_bins] of this point (staged)
  double* pred;                   // like obs
  int* live;                      // [2] of this point (staged): live events, injection set live
  int n_bins, n_pairs, pair, cx, cy;  // the current pair and its columns
  int first_tile, first_seg;      // the launches cover tiles / segments from here on (a set without bins is left out)
  int with_pe, with_inj;
};

__global__ __launch_bounds__(kBlock) void hist2d_tile_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) double w_lds[kTile];
  __shared__ __attribute__((aligned(16))) unsigned short code_lds[kTile];
  extern __shared__ __attribute__((aligned(16))) double cell_lds[];  // [n_bins n_bins]
  const int tile = a.first_tile + (int)blockIdx.x, n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double big = a.d.seg_max[seg];
  const long long tile_start = (long long)(tile - s.first_tile) * kTile;
  const int count = (int)(s.n - tile_start < kTile ? s.n - tile_start : kTile);  // (>= 1: the tile exists)
  const int j0 = (int)threadIdx.x * draw::kDrawPerLane;
  const unsigned n_bins = (unsigned)a.n_bins, n_cells = n_bins * n_bins;
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
  const unsigned short* codes_x = seg < a.d.n_ev ? a.bins_pe + ((long long)a.cx * a.d.n_ev + seg) * a.d.n_pe + tile_start : a.bins_inj + (long long)a.cx * a.d.n_inj + tile_start;
  const unsigned short* codes_y = seg < a.d.n_ev ? a.bins_pe + ((long long)a.cy * a.d.n_ev + seg) * a.d.n_pe + tile_start : a.bins_inj + (long long)a.cy * a.d.n_inj + tile_start;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const int j = j0 + q;
    unsigned joint = kNoCell;
    if (j < count) {
      const unsigned x = codes_x[j], y = codes_y[j];
      if (x < n_bins && y < n_bins) joint = x * n_bins + y;
    }
    code_lds[j] = (unsigned short)joint;
  }
  for (unsigned c = threadIdx.x; c < n_cells; c += kBlock) cell_lds[c] = 0.0;  // (this thread's own cells)
  __syncthreads();
  const unsigned me = threadIdx.x;
  const int end = (count + 3) & ~3;  // (the entries past count hold weight 0 and kNoCell)
  for (int i = 0; i < end; i += 4) {   // (no barrier in the loop: a cell has one owner)
    const uint2 k = *reinterpret_cast<const uint2*>(code_lds + i);
    const unsigned c0 = k.x & 0xFFFFu, c1 = k.x >> 16, c2 = k.y & 0xFFFFu, c3 = k.y >> 16;
    if ((c0 & (kBlock - 1)) == me && c0 < n_cells) cell_lds[c0] += w_lds[i];
    if ((c1 & (kBlock - 1)) == me && c1 < n_cells) cell_lds[c1] += w_lds[i + 1];
    if ((c2 & (kBlock - 1)) == me && c2 < n_cells) cell_lds[c2] += w_lds[i + 2];
    if ((c3 & (kBlock - 1)) == me && c3 < n_cells) cell_lds[c3] += w_lds[i + 3];
  }
  double* out = a.partial + (long long)tile * n_cells;
  for (unsigned c = threadIdx.x; c < n_cells; c += kBlock) out[c] = cell_lds[c];
}

__global__ __launch_bounds__(kBlock) void hist2d_merge_kernel(const Args a) {
  const int seg = a.first_seg + (int)blockIdx.x, n_cells = a.n_bins * a.n_bins;
  const int cell = (int)blockIdx.y * kBlock + (int)threadIdx.x;
  const double pv = a.v ? a.v[seg] : 1.0;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total = s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool live = total > 0.0 && total < __builtin_inf();
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    a.seg_dead[seg] = live ? 0 : 1;
    if (a.pair == 0 && pv != 0.0) {  // once per point, not once per pair
      if (!live && a.n_dead) a.n_dead[seg] += 1;
      if (live && a.v && a.vsum) a.vsum[seg] += pv;
    }
  }
  if (cell >= n_cells) return;
  double* q = a.share + (long long)seg * n_cells + cell;
  if (!live) {
    *q = __builtin_nan("");
    return;
  }
  const double* p = a.partial + (long long)s.first_tile * n_cells + cell;
  double sum = 0.0;
#pragma unroll 8
  for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * n_cells];
  const double quotient = sum / total;
  *q = quotient;
  if (a.hist && pv != 0.0) {
    double* h = a.hist + ((long long)seg * a.n_pairs + a.pair) * n_cells + cell;
    if (a.v) *h += draw::scaled(pv, quotient);
    else *h += quotient;
  }
}

__global__ __launch_bounds__(kBlock) void hist2d_mix_kernel(const Args a) {
  const int n_cells = a.n_bins * a.n_bins, cell = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  const int n_ev = a.d.n_ev;
  const bool inj_live = a.with_inj && a.seg_dead[n_ev] == 0;
  int n_live = 0;
  double sum = 0.0;
  if (a.with_pe)
    for (int e = 0; e < n_ev; ++e)  // (the flags are the same for every thread: no divergence)
      if (a.seg_dead[e] == 0) {
        ++n_live;
        if (cell < n_cells) sum += a.share[(long long)e * n_cells + cell];
      }
  if (a.pair == 0 && cell == 0) {
    a.live[0] = n_live;
    a.live[1] = inj_live ? 1 : 0;
  }
  if (cell >= n_cells) return;
  const long long at = (long long)a.pair * n_cells + cell;
  a.obs[at] = n_live > 0 ? sum / (double)n_live : __builtin_nan("");
  a.pred[at] = inj_live ? a.share[(long long)n_ev * n_cells + cell] : __builtin_nan("");
}

}  // namespace hist2d
}  // namespace gwi
