// gwi_draw.h -- weighted index draws from the per-sample log-weights the log-weight role of a scan chain leaves in HBM
// (include/gwi_engine.h: gwi_draw_indices; the reference's posterior-predictive branch, pipeline/analysis.py:321-355).
//
// A segment is one event's n_pe posterior samples or the injection set.  With M the largest finite log-weight of the segment's
// unmasked samples and w_j = exp(lw_j - M) (0 for masked or non-finite samples), a draw for the uniform u is the first sample with
// w_j > 0 whose inclusive prefix C_j exceeds u * C_last (the last such sample when rounding runs past the end, -1 when nothing has
// weight).  Three launches per hyper-parameter point, all ahead-of-time kernels (nothing here depends on the model's terms):
//
//   draw_tile_kernel    one workgroup per tile of kDrawTile samples (tiles never cross a segment): the tile's maximum and
//                       sum exp(lw - max) -- the online-softmax pair
//   draw_merge_kernel   one workgroup per segment: M, every tile's mass sum_t exp(max_t - M) and the inclusive prefix of the masses
//   draw_select_kernel  one workgroup per (segment, kDrawBatch uniforms): the first tile with mass whose prefix exceeds the target,
//                       then that tile alone is read again -- four consecutive samples per lane summed in order, a wave-level
//                       inclusive scan of the lane totals, LDS across the four waves -- and the first hit is found with a ballot
//
// Every sum has a fixed shape (lane order, butterfly, wave order, chunk order): the indices are a pure function of the inputs.  No
// atomics, nothing depends on which workgroup arrives first, and every store is a plain vector store.  The parallel prefixes are
// not monotone to the last bit, so a hit also requires weight (tile mass / sample weight) > 0: a sample without weight is never drawn.
#pragma once

#include <hip/hip_runtime.h>

namespace gwi {
namespace draw {

constexpr int kDrawBlock = 256;                        // four waves
constexpr int kDrawPerLane = 4;                        // consecutive samples per lane
constexpr int kDrawTile = kDrawBlock * kDrawPerLane;   // samples per tile
constexpr int kDrawBatch = 4;                          // uniforms per select workgroup
constexpr int kDrawNone = 0x7fffffff;

struct DrawArgs {
  const double* logw_pe;          // [n_ev][n_pe]  (without the sample-independent constant)
  const double* logw_inj;         // [n_inj]
  const unsigned char* mask_pe;   // nullptr: every sample may be drawn
  const unsigned char* mask_inj;
  double* tile_max;               // [n_ev * tiles_per_event + n_inj_tiles], PE tiles event-major, then the injection tiles
  double* tile_sum;
  double* tile_mass;
  double* tile_prefix;
  double* seg_max;                // [n_ev + 1]
  const double* u_pe;             // [n_ev][n_draw_pe] uniforms of this hyper-parameter point
  const double* u_inj;            // [n_draw_inj]
  int* idx_pe;                    // [n_ev][n_draw_pe]
  int* idx_inj;                   // [n_draw_inj]
  double log_const;               // added to every log-weight: a non-finite constant leaves nothing to draw, as on the host
  long long n_pe, n_inj;
  int n_ev, tiles_per_event, n_inj_tiles, n_draw_pe, n_draw_inj, batches_pe;
};

struct Segment {
  const double* lw;
  const unsigned char* mask;
  long long n;
  int first_tile, n_tiles;
};

__device__ inline Segment segment_of(const DrawArgs& a, int seg) {
  if (seg < a.n_ev)
    return Segment{a.logw_pe + (long long)seg * a.n_pe, a.mask_pe ? a.mask_pe + (long long)seg * a.n_pe : nullptr, a.n_pe, seg * a.tiles_per_event, a.tiles_per_event};
  return Segment{a.logw_inj, a.mask_inj, a.n_inj, a.n_ev * a.tiles_per_event, a.n_inj_tiles};
}

// log-weight of sample j of a segment, or -inf when it cannot be drawn (masked, -inf, +inf, NaN)
__device__ inline double live_log_weight(const Segment& s, long long j, double log_const) {
  const double v = s.lw[j] + log_const;
  const bool on = s.mask ? s.mask[j] != 0 : true;
  return on && fabs(v) < __builtin_inf() ? v : -__builtin_inf();
}

// v q rounded once on its own: never contracted into the addition that follows
__device__ inline double scaled(double v, double q) {
#pragma clang fp contract(off)
  return v * q;
}

struct OpMax {
  template <class T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct OpMin {
  template <class T>
  __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};
struct OpAdd {
  template <class T>
  __device__ T operator()(T a, T b) const { return a + b; }
};

// butterfly over the 64 lanes, then the four waves' values in wave order: every thread gets the same bits
template <class T, class Op>
__device__ inline T block_reduce(T v, T* lds, Op op) {
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o));
  __syncthreads();  // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = lds[0];
  for (int w = 1; w < kDrawBlock / 64; ++w) r = op(r, lds[w]);
  return r;
}

// inclusive prefix over the block's threads; total = the block's sum (the same bits in every thread)
__device__ inline double block_inclusive_scan(double v, double* lds, double* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  double off = 0.0, all = 0.0;
  for (int w = 0; w < kDrawBlock / 64; ++w) {
    if (w < wave) off += lds[w];
    all += lds[w];
  }
  *total = all;
  return off + v;
}

__global__ __launch_bounds__(kDrawBlock) void draw_tile_kernel(const DrawArgs a) {
  __shared__ double lds[kDrawBlock / 64];
  const int b = blockIdx.x, n_pe_tiles = a.n_ev * a.tiles_per_event;
  const int seg = b < n_pe_tiles ? b / a.tiles_per_event : a.n_ev;
  const Segment s = segment_of(a, seg);
  const long long start = (long long)(b - s.first_tile) * kDrawTile + (long long)threadIdx.x * kDrawPerLane;
  double v[kDrawPerLane], m = -__builtin_inf();
#pragma unroll
  for (int c = 0; c < kDrawPerLane; ++c) {
    v[c] = start + c < s.n ? live_log_weight(s, start + c, a.log_const) : -__builtin_inf();
    m = fmax(m, v[c]);
  }
  m = block_reduce(m, lds, OpMax());
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < kDrawPerLane; ++c)
    if (v[c] > -__builtin_inf()) sum += exp(v[c] - m);
  sum = block_reduce(sum, lds, OpAdd());
  if (threadIdx.x == 0) {
    a.tile_max[b] = m;
    a.tile_sum[b] = sum;
  }
}

__global__ __launch_bounds__(kDrawBlock) void draw_merge_kernel(const DrawArgs a) {
  __shared__ double lds[kDrawBlock / 64];
  const int seg = blockIdx.x;
  const Segment s = segment_of(a, seg);
  double big = -__builtin_inf();
  for (int t = threadIdx.x; t < s.n_tiles; t += kDrawBlock) big = fmax(big, a.tile_max[s.first_tile + t]);
  big = block_reduce(big, lds, OpMax());
  double carry = 0.0;
  for (int base = 0; base < s.n_tiles; base += kDrawBlock) {  // (the trip count is the same for every thread)
    const int t = base + (int)threadIdx.x;
    double mass = 0.0;
    if (t < s.n_tiles && a.tile_sum[s.first_tile + t] > 0.0) mass = a.tile_sum[s.first_tile + t] * exp(a.tile_max[s.first_tile + t] - big);
    double total;
    const double incl = block_inclusive_scan(mass, lds, &total);
    if (t < s.n_tiles) {
      a.tile_mass[s.first_tile + t] = mass;
      a.tile_prefix[s.first_tile + t] = carry + incl;
    }
    carry += total;
  }
  if (threadIdx.x == 0) a.seg_max[seg] = big;
}

__global__ __launch_bounds__(kDrawBlock) void draw_select_kernel(const DrawArgs a) {
  __shared__ double lds[kDrawBlock / 64];
  __shared__ int ldi[kDrawBlock / 64];
  const int b = blockIdx.x, n_pe_blocks = a.n_ev * a.batches_pe;
  const bool pe = b < n_pe_blocks;
  const int seg = pe ? b / a.batches_pe : a.n_ev, batch = pe ? b % a.batches_pe : b - n_pe_blocks;
  const int n_draw = pe ? a.n_draw_pe : a.n_draw_inj;
  const double* u = pe ? a.u_pe + (long long)seg * a.n_draw_pe : a.u_inj;
  int* out = pe ? a.idx_pe + (long long)seg * a.n_draw_pe : a.idx_inj;
  const Segment s = segment_of(a, seg);
  const double big = a.seg_max[seg];
  const double* prefix = a.tile_prefix + s.first_tile;
  const double* mass = a.tile_mass + s.first_tile;
  const double c_last = s.n_tiles > 0 ? prefix[s.n_tiles - 1] : 0.0;
  for (int q = 0; q < kDrawBatch; ++q) {
    const int d = batch * kDrawBatch + q;
    if (d >= n_draw) break;  // (the same for every thread of the workgroup, like every branch around a barrier below)
    if (!(c_last > 0.0)) {
      if (threadIdx.x == 0) out[d] = -1;
      continue;
    }
    const double target = u[d] * c_last;
    // the tile: the first one with mass whose prefix exceeds the target, else the last one with mass
    int first = kDrawNone, last = -1;
    for (int t = threadIdx.x; t < s.n_tiles; t += kDrawBlock)
      if (mass[t] > 0.0) {
        last = t;
        if (first == kDrawNone && prefix[t] > target) first = t;
      }
    first = block_reduce(first, ldi, OpMin());
    last = block_reduce(last, ldi, OpMax());
    const int tile = first != kDrawNone ? first : last;  // c_last > 0: some tile has mass
    const double rest = target - (tile > 0 ? prefix[tile - 1] : 0.0);
    // ... and the sample inside it
    const int j0 = (int)threadIdx.x * kDrawPerLane;
    const long long start = (long long)tile * kDrawTile + j0;
    double w[kDrawPerLane], run = 0.0;
#pragma unroll
    for (int c = 0; c < kDrawPerLane; ++c) {
      const double v = start + c < s.n ? live_log_weight(s, start + c, a.log_const) : -__builtin_inf();
      w[c] = v > -__builtin_inf() ? exp(v - big) : 0.0;
      run += w[c];
    }
    double total;
    const double before = block_inclusive_scan(run, lds, &total) - run;
    int hit = kDrawNone, live = -1;
    double c_j = before;
#pragma unroll
    for (int c = 0; c < kDrawPerLane; ++c) {
      c_j += w[c];
      if (w[c] > 0.0) {
        live = j0 + c;
        if (hit == kDrawNone && c_j > rest) hit = j0 + c;
      }
    }
    // the first lane of a wave with a hit holds the wave's smallest index: lanes hold ascending samples
    const unsigned long long any = __ballot(hit != kDrawNone);
    const int wave_hit = any ? __shfl(hit, __ffsll((long long)any) - 1) : kDrawNone;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ldi[threadIdx.x >> 6] = wave_hit;
    __syncthreads();
    int sel = kDrawNone;
    for (int wv = kDrawBlock / 64 - 1; wv >= 0; --wv)
      if (ldi[wv] != kDrawNone) sel = ldi[wv];
    if (sel == kDrawNone) sel = block_reduce(live, ldi, OpMax());  // rounding ran past the tile's end (sel is uniform: so is the branch)
    if (threadIdx.x == 0) out[d] = sel >= 0 ? (int)((long long)tile * kDrawTile + sel) : -1;
  }
}

inline long long tiles_of(long long n) { return (n + kDrawTile - 1) / kDrawTile; }

}  // namespace draw
}  // namespace gwi
