// gwi_boot.h -- bootstrap replicates of the inner importance sums: for ONE hyper-parameter point at a time and every segment, the sums
// A_b = sum_i c_ib w_i of B Poisson-bootstrap replicates of the segment's samples, with the same resampling at every point
// (include/gwi_engine.h: gwi_set_bootstrap, gwi_point_bootstrap; the NumPy statement is gwinferno_amd/draws.py: bootstrap_counts,
// point_bootstrap_reference; what the host makes of the sums is draws.bootstrap_likelihood; the contract is DESIGN 8n).
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's; M and S are draw_tile_kernel's / draw_merge_kernel's for the point.
// w_i = exp(lw_i - M), 0 for a sample that is masked or not finite.  Sample i of a segment has the global index e n_pe + j (PE sample j
// of event e) or n_ev n_pe + j (injection j); replicate b takes word b % 4 of the Philox4x32-10 block with the counter (index low,
// index high, b / 4, kTag) and the seed's halves as the key (gwi_spinprior.h's generator), and the count c_ib is the number of entries
// of kPoisson1 that are <= the word: a Poisson(1) variate by inversion, in integer comparisons only, so that host and device agree on
// every count in every bit.  kTag is disjoint from gwi_mock.h's 0x4D4F4B00 + b and 0x4D4F4B10 + b (b < 4), gwi_resample.h's
// 0x52534D50, gwi_popdraw.h's 0x504F5044 and the 2 t, 2 t + 1 < 2^17 of gwi_spinprior.h.  Two launches per point:
//
//   boot_tile_kernel    one workgroup per tile of kTile samples (tiles never cross a segment).  The tile's weights are staged in LDS
//                       once (8 KB; no exp() after that) beside a byte per sample that says whether it is unmasked.  A thread owns one
//                       group of four replicates -- one Philox block per sample -- and one slice of kSlice = 128 consecutive samples: it
//                       walks the slice in sample order with four running doubles (one convert, one fused multiply-add per sample and
//                       replicate) and four running integer counts in registers; the 32 lanes that share a slice read the same LDS
//                       address (a broadcast).  8 slices x 32 groups = 128 replicates per pass; more replicates take more passes.  The
//                       8 slice sums of a replicate are added in slice order through LDS, and the tile's A_b -- on the first point of
//                       a call also C_b = sum of c_ib over the unmasked samples, finite or not -- go to the partials [n_tiles][B]
//   boot_merge_kernel   one workgroup per segment: thread t adds replicates t, t + 256, ... over the segment's tiles in tile order and
//                       writes the point's row of the staging buffer, (M, S) of the segment and the flag 1 for a segment without weight
//                       (hist_merge_kernel's rule on S: NaN sums, flag set); on the first point also the int64 counts
//
// A replicate's sum has ONE shape -- sample order within a slice of fixed length, slice order, tile order -- that involves neither the
// number of replicates of the call nor its first replicate (a thread computes the whole block of an absolute group b / 4 and drops the
// words outside the call's range), so the bits of A_b are a pure function of (theta, seed, b, masks).  A sample past the segment's end
// or masked would add c * 0 = 0 and counts for nothing, which changes no bit: such samples are skipped.  No atomics, no scratch, every store is a
// plain vector store.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"
#include "gwi_spinprior.h"

namespace gwi {
namespace boot {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kSlices = 8;
constexpr int kSlice = kTile / kSlices;          // 128 consecutive samples
constexpr int kGroups = kBlock / kSlices;        // 32 groups of four replicates per pass
constexpr int kPerPass = 4 * kGroups;            // 128 replicates
constexpr int kMaxReplicates = 1024;             // per call
constexpr int kMaxReplicate = 1 << 20;           // first_replicate + n_replicates <= this
constexpr unsigned kTag = 0x424F4F54u;           // counter word 3 ("BOOT")
constexpr int kStats = 2;
static_assert(kSlices * kGroups == kBlock && kSlices * kSlice == kTile, "slices and groups tile the workgroup and the tile");

// kPoisson1[j] = floor(2^32 F(j)), F the Poisson(1) CDF, j = 0 ... 12: the table ends with the largest word, which no later entry
// could exceed.  The Poisson(1) count of a 32-bit word is the number of entries that are <= it: thirteen integer comparisons, unrolled
// into literals
constexpr int kPoisson1Size = 13;
__host__ __device__ constexpr int poisson1(unsigned u) {
  constexpr unsigned kPoisson1[kPoisson1Size] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u,
                                                 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u};
  int c = 0;
  for (int j = 0; j < kPoisson1Size; ++j) c += u >= kPoisson1[j] ? 1 : 0;
  return c;
}
static_assert(poisson1(0u) == 0 && poisson1(1580030167u) == 0 && poisson1(1580030168u) == 1 && poisson1(4294967294u) == 12 && poisson1(4294967295u) == 13, "counts by inversion");

struct Args {
  draw::DrawArgs d;       // the segments, the masks, log_const, seg_max and tile_prefix of this point
  double* tile_sum;       // [n_tiles][n_rep], tiles numbered as in DrawArgs
  int* tile_count;        // [n_tiles][n_rep]
  double* sums;           // [n_ev + 1][n_rep]: the point's row of the staging buffer
  double* stats;          // [n_ev + 1][kStats]
  int* dead;              // [n_ev + 1]
  long long* counts;      // [n_ev + 1][n_rep], written when want_counts
  unsigned long long seed;
  int n_rep, first_rep, want_counts;
};

__global__ __launch_bounds__(kBlock) void boot_tile_kernel(const Args a) {
  __shared__ double w[kTile];
  __shared__ unsigned char open[kTile];
  __shared__ double part[kSlices][kPerPass];
  __shared__ int part_c[kSlices][kPerPass];
  const int tile = (int)blockIdx.x, tid = (int)threadIdx.x, n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  const int seg = tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const long long tile_start = (long long)(tile - s.first_tile) * kTile;
  const long long rest = s.n - tile_start;
  const int n_here = rest < kTile ? (int)rest : kTile;  // samples of the segment in this tile (>= 1)
  const double big = a.d.seg_max[seg];
  for (int i = tid; i < kTile; i += kBlock) {
    double wi = 0.0;
    unsigned char on = 0;
    if (i < n_here) {
      const double v = draw::live_log_weight(s, tile_start + i, a.d.log_const);
      wi = v > -__builtin_inf() ? exp(v - big) : 0.0;
      on = s.mask ? s.mask[tile_start + i] != 0 : 1;
    }
    w[i] = wi;
    open[i] = on;
  }
  __syncthreads();
  const int slice = tid / kGroups, lane_group = tid % kGroups;
  const int first_group = a.first_rep >> 2, last_group = (a.first_rep + a.n_rep - 1) >> 2;
  const int i0 = slice * kSlice, i1 = i0 + kSlice < n_here ? i0 + kSlice : n_here;
  const unsigned long long index0 = (unsigned long long)(seg < a.d.n_ev ? (long long)seg * a.d.n_pe : (long long)a.d.n_ev * a.d.n_pe) + (unsigned long long)tile_start;
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
  for (int g0 = first_group; g0 <= last_group; g0 += kGroups) {  // (the trip count is the same for every thread)
    const int g = g0 + lane_group;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[4] = {0, 0, 0, 0};
    if (g <= last_group)
      for (int i = i0; i < i1; ++i) {
        const double wi = w[i];
        const int on = open[i];
        if (!on) continue;  // a masked sample has no weight and no count (the same for the lanes of a slice)
        const unsigned long long index = index0 + (unsigned long long)i;
        const spinprior::U4 r = spinprior::philox4x32_10(spinprior::U4{(unsigned)index, (unsigned)(index >> 32), (unsigned)g, kTag}, k0, k1);
        const int c0 = poisson1(r.x), c1 = poisson1(r.y), c2 = poisson1(r.z), c3 = poisson1(r.w);
        acc[0] = __builtin_fma((double)c0, wi, acc[0]);
        acc[1] = __builtin_fma((double)c1, wi, acc[1]);
        acc[2] = __builtin_fma((double)c2, wi, acc[2]);
        acc[3] = __builtin_fma((double)c3, wi, acc[3]);
        cnt[0] += c0;
        cnt[1] += c1;
        cnt[2] += c2;
        cnt[3] += c3;
      }
    __syncthreads();  // the previous pass has read part
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      part[slice][4 * lane_group + q] = acc[q];
      part_c[slice][4 * lane_group + q] = cnt[q];
    }
    __syncthreads();
    if (tid < kPerPass) {
      const int r = 4 * g0 + tid - a.first_rep;  // the replicate's place in the call
      if (r >= 0 && r < a.n_rep) {
        double sum = part[0][tid];
        int c = part_c[0][tid];
#pragma unroll
        for (int sl = 1; sl < kSlices; ++sl) {
          sum += part[sl][tid];
          c += part_c[sl][tid];
        }
        a.tile_sum[(long long)tile * a.n_rep + r] = sum;
        if (a.want_counts) a.tile_count[(long long)tile * a.n_rep + r] = c;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void boot_merge_kernel(const Args a) {
  const int seg = (int)blockIdx.x, tid = (int)threadIdx.x;
  const draw::Segment s = draw::segment_of(a.d, seg);
  const double total_w = s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool live = total_w > 0.0 && total_w < __builtin_inf();  // hist_merge_kernel's rule
  double* out = a.sums + (long long)seg * a.n_rep;
  for (int r = tid; r < a.n_rep; r += kBlock) {
    const double* p = a.tile_sum + (long long)s.first_tile * a.n_rep + r;
    double sum = 0.0;
#pragma unroll 4
    for (int t = 0; t < s.n_tiles; ++t) sum += p[(long long)t * a.n_rep];
    out[r] = live ? sum : __builtin_nan("");
    if (a.want_counts) {
      const int* pc = a.tile_count + (long long)s.first_tile * a.n_rep + r;
      long long c = 0;
#pragma unroll 4
      for (int t = 0; t < s.n_tiles; ++t) c += pc[(long long)t * a.n_rep];
      a.counts[(long long)seg * a.n_rep + r] = c;
    }
  }
  if (tid == 0) {
    a.stats[(long long)seg * kStats] = a.d.seg_max[seg];
    a.stats[(long long)seg * kStats + 1] = total_w;
    a.dead[seg] = live ? 0 : 1;
  }
}

}  // namespace boot
}  // namespace gwi
