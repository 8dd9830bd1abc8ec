// gwi_tail.h -- per-point tails of the inner importance sums: for ONE hyper-parameter point at a time and every segment, the m largest live
// log-weights in ascending order, the numbers that define the cut-off below them and the sum of everything outside the tail
// (include/gwi_engine.h: gwi_set_tail_sizes, gwi_point_tails; the NumPy statement is gwinferno_amd/draws.py: point_tails_reference; the
// Pareto fit of the tail is the host's, draws.pareto_tail_fit; the contract is DESIGN 8m).
//
// Segments, tiles, masks and live_log_weight() are gwi_draw.h's.  A live sample's value l_j = lw_j + log_const is finite.  It is mapped
// to an order-preserving uint64 key -- every bit of a negative flipped, the sign bit of a non-negative set, -0.0 taken as +0.0 first --
// so that values compare as keys, no live key is 0, and key 0 stands for -inf.  With m the segment's tail size (m_pe or m_inj) the key
// T of the m-th largest live value v* is found by a most-significant-digit radix selection in kPasses passes of 11, 11, 11, 11, 10, 10
// bits, two launches per pass, whatever the data are:
//
//   tail_hist_kernel     one workgroup per tile of kTile samples (tiles never cross a segment): the histogram of the pass's digit over
//                        the tile's live keys that match the segment's prefix so far, counted with integer adds in LDS
//   tail_pick_kernel     one workgroup per segment: adds the tiles' histograms, finds the digit that holds the remaining rank from the
//                        top, appends it to the prefix and lowers the rank by the keys above the digit.  A segment with fewer than m
//                        live samples is marked short: its T is 0, every live value lies above it
//
// and two more collect:
//
//   tail_collect_kernel  one workgroup per tile: n_live, n_gt = #(key > T), n_eq = #(key == T), the largest key below T, and the tile's
//                        part of body = sum over key < T of exp(l_j - M) -- four consecutive samples per lane in order, butterfly, wave
//                        order; every key > T goes to the tile's own 1 024 candidate slots (which one: an integer LDS counter)
//   tail_merge_kernel    one workgroup per segment: the tiles' counts, the largest key below, body in tile order; the candidates of all
//                        tiles and m - n_gt copies of T into LDS, padded to a power of two, a bitonic sort, the keys mapped back; the
//                        point's rows of tail, stats = (M, S, body, below_max) and counts = (n_live, n_gt, n_eq, dead)
//
// M and S are draw_merge_kernel's; a segment is dead by hist_merge_kernel's rule on S and then has an all -inf tail, zero counts and NaN
// body.  tail, counts and below_max are exact functions of the inputs: the slot a candidate lands in depends on arrival, the sorted
// result does not.  body has a fixed shape (lane order, butterfly, wave order, tile order).  No floating-point atomics, every store is
// a plain vector store; no scratch.  The candidates reuse the histograms' memory: kHistStride ints = kTile keys per tile.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"

namespace gwi {
namespace tail {

constexpr int kBlock = draw::kDrawBlock;
constexpr int kTile = draw::kDrawTile;
constexpr int kPasses = 6;
constexpr int kMaxDigits = 2048;            // 11 bits
constexpr int kHistStride = kMaxDigits;     // ints per tile: one pass's histogram, then kTile candidate keys
constexpr int kMaxTail = 4096;              // keys the merge sorts in LDS (32 KB)
constexpr int kTileInts = 4;                // n_live, n_gt, n_eq, (unused)
constexpr int kStats = 4, kCounts = 4;
static_assert(kHistStride * sizeof(int) == kTile * sizeof(unsigned long long), "a tile's candidates fit its histogram");

typedef unsigned long long u64;

__host__ __device__ constexpr int digit_bits(int pass) { return pass < 4 ? 11 : 10; }
__host__ __device__ constexpr int digit_shift(int pass) { return pass < 4 ? 53 - 11 * pass : 10 * (5 - pass); }
static_assert(digit_shift(0) + digit_bits(0) == 64 && digit_shift(kPasses - 1) == 0 && digit_shift(3) == digit_shift(4) + digit_bits(4), "the digits tile the key");

struct Args {
  draw::DrawArgs d;   // the segments, the masks, log_const, seg_max and tile_prefix of this point
  u64* prefix;        // [n_ev + 1] the digits picked so far; T after the last pass
  int* rank;          // [n_ev + 1][2] the rank from the top among the keys that match the prefix; 1 when the segment is short
  int* hist;          // [n_tiles][kHistStride], tiles numbered as in DrawArgs; after the selection the tiles' candidate keys
  double* tile_body;  // [n_tiles]
  u64* tile_below;    // [n_tiles]
  int* tile_counts;   // [n_tiles][kTileInts]
  double* tail;       // [n_ev m_pe + m_inj]: the point's row of the staging buffer
  double* stats;      // [n_ev + 1][kStats]
  int* counts;        // [n_ev + 1][kCounts]
  int m_pe, m_inj, pass;
};

__device__ inline int tail_size(const Args& a, int seg) { return seg < a.d.n_ev ? a.m_pe : a.m_inj; }

// the key of a finite value
__device__ inline u64 key_of(double v) {
  const u64 b = v == 0.0 ? 0ull : (u64)__double_as_longlong(v);
  return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
// ... and back; 0 is -inf
__device__ inline double value_of(u64 k) {
  if (k == 0) return -__builtin_inf();
  return __longlong_as_double((long long)(k >> 63 ? k & 0x7fffffffffffffffull : ~k));
}

// the keys of the thread's four consecutive samples of a tile, 0 where there is no live sample; the values beside them
__device__ inline void load_keys(const Args& a, const draw::Segment& s, int tile, u64 (&key)[draw::kDrawPerLane], double (&v)[draw::kDrawPerLane]) {
  const long long start = (long long)(tile - s.first_tile) * kTile + (long long)threadIdx.x * draw::kDrawPerLane;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    v[q] = start + q < s.n ? draw::live_log_weight(s, start + q, a.d.log_const) : -__builtin_inf();
    key[q] = v[q] > -__builtin_inf() ? key_of(v[q]) : 0ull;
  }
}

__device__ inline int segment_of_tile(const Args& a, int tile) {
  const int n_pe_tiles = a.d.n_ev * a.d.tiles_per_event;
  return tile < n_pe_tiles ? tile / a.d.tiles_per_event : a.d.n_ev;
}

// inclusive prefix of one int per thread; total = the block's sum
__device__ inline int block_inclusive_scan_int(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  __syncthreads();  // the previous use of lds is over
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  int off = 0, all = 0;
  for (int w = 0; w < kBlock / 64; ++w) {
    if (w < wave) off += lds[w];
    all += lds[w];
  }
  *total = all;
  return off + v;
}

__global__ __launch_bounds__(kBlock) void tail_hist_kernel(const Args a) {
  __shared__ int h[kMaxDigits];
  const int tile = (int)blockIdx.x, seg = segment_of_tile(a, tile);
  const int bits = digit_bits(a.pass), shift = digit_shift(a.pass), n_digits = 1 << bits;
  if (a.pass > 0 && a.rank[2 * seg + 1]) return;  // a short segment: nothing is picked any more (the same for every thread)
  const draw::Segment s = draw::segment_of(a.d, seg);
  for (int i = threadIdx.x; i < n_digits; i += kBlock) h[i] = 0;
  __syncthreads();
  const u64 prefix = a.pass > 0 ? a.prefix[seg] : 0ull;
  u64 key[draw::kDrawPerLane];
  double v[draw::kDrawPerLane];
  load_keys(a, s, tile, key, v);
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    const bool match = key[q] != 0 && (a.pass == 0 || key[q] >> (shift + bits) == prefix);
    if (match) atomicAdd(&h[(int)(key[q] >> shift) & (n_digits - 1)], 1);
  }
  __syncthreads();
  int* out = a.hist + (long long)tile * kHistStride;
  for (int i = threadIdx.x; i < n_digits; i += kBlock) out[i] = h[i];
}

__global__ __launch_bounds__(kBlock) void tail_pick_kernel(const Args a) {
  __shared__ int cnt[kMaxDigits];
  __shared__ int lds[kBlock / 64];
  const int seg = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int bits = digit_bits(a.pass), n_digits = 1 << bits, per = n_digits / kBlock;  // 8 or 4 digits per thread
  if (a.pass > 0 && a.rank[2 * seg + 1]) return;  // (the same for every thread)
  const draw::Segment s = draw::segment_of(a.d, seg);
  const int r = a.pass > 0 ? a.rank[2 * seg] : tail_size(a, seg);
  const u64 prefix = a.pass > 0 ? a.prefix[seg] : 0ull;
  // digit tid + kBlock q of every tile, added over the tiles (integers: the order does not matter)
  int acc[kMaxDigits / kBlock];
#pragma unroll
  for (int q = 0; q < kMaxDigits / kBlock; ++q) acc[q] = 0;
  const int* p = a.hist + (long long)s.first_tile * kHistStride + tid;
#pragma unroll 4
  for (int t = 0; t < s.n_tiles; ++t)
#pragma unroll
    for (int q = 0; q < kMaxDigits / kBlock; ++q)
      if (q < per) acc[q] += p[(long long)t * kHistStride + q * kBlock];
#pragma unroll
  for (int q = 0; q < kMaxDigits / kBlock; ++q)
    if (q < per) cnt[tid + q * kBlock] = acc[q];
  __syncthreads();
  // thread tid owns the digits [tid per, (tid + 1) per): the keys above them, then the walk down from the top one
  int own = 0;
  for (int i = 0; i < per; ++i) own += cnt[tid * per + i];
  int total;
  const int incl = block_inclusive_scan_int(own, lds, &total);
  if (r > total) {  // fewer keys than the rank: only ever in pass 0, where the segment has fewer than m live samples
    if (tid == 0) {
      a.prefix[seg] = 0ull;
      a.rank[2 * seg] = 0;
      a.rank[2 * seg + 1] = 1;
    }
    return;
  }
  int above = total - incl;
  for (int i = per - 1; i >= 0; --i) {
    const int dgt = tid * per + i, c = cnt[dgt];
    if (above < r && r <= above + c) {  // (true for one digit of one thread)
      a.prefix[seg] = prefix << bits | (u64)dgt;
      a.rank[2 * seg] = r - above;
      a.rank[2 * seg + 1] = 0;
    }
    above += c;
  }
}

__global__ __launch_bounds__(kBlock) void tail_collect_kernel(const Args a) {
  __shared__ double lds[kBlock / 64];
  __shared__ int ldi[kBlock / 64];
  __shared__ u64 ldk[kBlock / 64];
  __shared__ int n_slots;
  const int tile = (int)blockIdx.x, seg = segment_of_tile(a, tile);
  const draw::Segment s = draw::segment_of(a.d, seg);
  const u64 t_key = a.prefix[seg];
  const double big = a.d.seg_max[seg];
  if (threadIdx.x == 0) n_slots = 0;
  __syncthreads();
  u64 key[draw::kDrawPerLane], below = 0ull, *cand = reinterpret_cast<u64*>(a.hist + (long long)tile * kHistStride);
  double v[draw::kDrawPerLane], body = 0.0;
  load_keys(a, s, tile, key, v);
  int n_live = 0, n_gt = 0, n_eq = 0;
#pragma unroll
  for (int q = 0; q < draw::kDrawPerLane; ++q) {
    if (key[q] == 0) continue;
    ++n_live;
    if (key[q] > t_key) {
      ++n_gt;
      cand[atomicAdd(&n_slots, 1)] = key[q];  // (at most kTile live samples per tile: the slot exists)
    } else if (key[q] == t_key) {
      ++n_eq;
    } else {
      body += exp(v[q] - big);
      below = key[q] > below ? key[q] : below;
    }
  }
  body = draw::block_reduce(body, lds, draw::OpAdd());
  below = draw::block_reduce(below, ldk, draw::OpMax());
  n_live = draw::block_reduce(n_live, ldi, draw::OpAdd());
  n_gt = draw::block_reduce(n_gt, ldi, draw::OpAdd());
  n_eq = draw::block_reduce(n_eq, ldi, draw::OpAdd());
  if (threadIdx.x == 0) {
    a.tile_body[tile] = body;
    a.tile_below[tile] = below;
    int* c = a.tile_counts + (long long)tile * kTileInts;
    c[0] = n_live;
    c[1] = n_gt;
    c[2] = n_eq;
    c[3] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void tail_merge_kernel(const Args a) {
  __shared__ u64 keys[kMaxTail];
  __shared__ int upto[kBlock];  // the inclusive prefix of n_gt over a chunk of kBlock tiles
  __shared__ int ldi[kBlock / 64];
  __shared__ u64 ldk[kBlock / 64];
  const int seg = (int)blockIdx.x, tid = (int)threadIdx.x, m = tail_size(a, seg);
  const draw::Segment s = draw::segment_of(a.d, seg);
  const u64 t_key = a.prefix[seg];
  const double total_w = s.n_tiles > 0 ? a.d.tile_prefix[s.first_tile + s.n_tiles - 1] : 0.0;
  const bool live = total_w > 0.0 && total_w < __builtin_inf();  // hist_merge_kernel's rule
  double* out = a.tail + (seg < a.d.n_ev ? (long long)seg * a.m_pe : (long long)a.d.n_ev * a.m_pe);
  if (!live) {  // (the same for every thread)
    for (int i = tid; i < m; i += kBlock) out[i] = -__builtin_inf();
    if (tid == 0) {
      double* st = a.stats + (long long)seg * kStats;
      st[0] = a.d.seg_max[seg];
      st[1] = total_w;
      st[2] = __builtin_nan("");
      st[3] = -__builtin_inf();
      int* c = a.counts + (long long)seg * kCounts;
      c[0] = c[1] = c[2] = 0;
      c[3] = 1;
    }
    return;
  }
  int n_live = 0, n_gt = 0, n_eq = 0, placed = 0;
  u64 below = 0ull;
  for (int t0 = 0; t0 < s.n_tiles; t0 += kBlock) {  // (the trip count is the same for every thread)
    const int t = t0 + tid;
    const int* c = a.tile_counts + (long long)(s.first_tile + t) * kTileInts;
    const int c_live = t < s.n_tiles ? c[0] : 0, c_gt = t < s.n_tiles ? c[1] : 0, c_eq = t < s.n_tiles ? c[2] : 0;
    const u64 c_below = t < s.n_tiles ? a.tile_below[s.first_tile + t] : 0ull;
    n_live += draw::block_reduce(c_live, ldi, draw::OpAdd());
    n_eq += draw::block_reduce(c_eq, ldi, draw::OpAdd());
    const u64 chunk_below = draw::block_reduce(c_below, ldk, draw::OpMax());
    below = chunk_below > below ? chunk_below : below;
    int chunk;
    upto[tid] = block_inclusive_scan_int(c_gt, ldi, &chunk);
    __syncthreads();
    // candidate e of the chunk lies in the first tile whose inclusive prefix exceeds e
    for (int e = tid; e < chunk; e += kBlock) {
      int lo = 0, hi = kBlock - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (upto[mid] > e) hi = mid;
        else lo = mid + 1;
      }
      const int at = e - (lo ? upto[lo - 1] : 0), dst = placed + e;  // at < the tile's n_gt <= kTile
      if (dst < m && dst < kMaxTail) keys[dst] = reinterpret_cast<const u64*>(a.hist + (long long)(s.first_tile + t0 + lo) * kHistStride)[at];
    }
    placed += chunk;
    n_gt += chunk;
    __syncthreads();  // upto is rewritten by the next chunk
  }
  // n_gt < m by the selection; the rest of the tail is copies of v*, the padding sorts behind everything
  int size = 1;
  while (size < m) size <<= 1;
  for (int i = (placed < m ? placed : m) + tid; i < size && i < kMaxTail; i += kBlock) keys[i] = i < m ? t_key : ~0ull;
  __syncthreads();
  for (int k = 2; k <= size; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < size; i += kBlock) {
        const int partner = i ^ j;
        if (partner > i) {
          const u64 x = keys[i], y = keys[partner];
          const bool up = (i & k) == 0;
          if (up ? x > y : x < y) {
            keys[i] = y;
            keys[partner] = x;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < m; i += kBlock) out[i] = value_of(keys[i]);
  if (tid == 0) {
    double body = 0.0;
#pragma unroll 8
    for (int t = 0; t < s.n_tiles; ++t) body += a.tile_body[s.first_tile + t];
    double* st = a.stats + (long long)seg * kStats;
    st[0] = a.d.seg_max[seg];
    st[1] = total_w;
    st[2] = body;
    st[3] = value_of(below);
    int* c = a.counts + (long long)seg * kCounts;
    c[0] = n_live;
    c[1] = n_gt;
    c[2] = n_eq;
    c[3] = 0;
  }
}

}  // namespace tail
}  // namespace gwi
