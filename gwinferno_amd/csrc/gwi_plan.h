// gwi_plan.h -- launch planning of gwi_create as host arithmetic: the GWI_* knobs, the launch geometry of the scan and tail
// kernels (single evaluations and batched launches) and the replica count of the gradient rows in LDS.  No HIP in here: plain
// C++17, so that the rules -- which fix the summation order, and with it the bits, of every evaluation -- run in a CPU test
// (tests/test_plan_cpu.py).  gwi_engine.hip ties the constants below to gwi_device.h with static_asserts.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace gwi_plan {

constexpr int kBlock = 256;             // threads per scan workgroup
constexpr unsigned kGeomTilesBits = 7;  // bits of the tiles-per-event field in the scan's packed geometry word (ScanHead::geom)
constexpr int kRegularRepShift = 4;     // 16 gradient-row replicas in the regular (non-SAFE) scan kernels
constexpr int kPolyStride = 256 + 1;  // doubles between the four power-basis arrays of the spline values (GWI_MAX_THETA + 1)
// the scan receives its tile sizes in 16 bits each (ScanHead::chunks): exact below 32 768 samples, multiples of 256 above
inline bool chunk_packs(long long c) { return c > 0 && (c < 32768 || (c % 256 == 0 && c / 256 < 32768)); }

// One GWI_* variable: whether it is set at all (some rules ask only that) and its text through atoi / atoll / atof.
template <class T>
struct Knob {
  bool set = false;
  T v{};
  bool off() const { return set && v == 0; }
  bool on() const { return set && v != 0; }
};

// Every variable gwi_create reads for itself: member of Knobs, type (int: atoi, long long: atoll, double: atof), name.
#define GWI_PLAN_KNOBS(X)                                                                                                                                        \
  X(force_generic, int, "GWI_FORCE_GENERIC")            /* tests / measurements: the generic kernel for a model that has a compiled chain */                     \
  X(force_jit, int, "GWI_FORCE_JIT")                    /* ... a run-time compiled chain for a model that has an ahead-of-time one */                            \
  X(jit, int, "GWI_JIT")                                /* 0: nothing is compiled at run time (scan chains, matrix-core instantiations) */                       \
  X(samples_per_lane, int, "GWI_SAMPLES_PER_LANE")      /* 1 or 2 samples per lane and trip, whatever the rules say */                                           \
  X(quiet, int, "GWI_QUIET")                            /* set: no warning when a model falls to the generic kernel */                                           \
  X(spin_wait, int, "GWI_SPIN_WAIT")                    /* 0: waits yield instead of spinning */                                                                 \
  X(max_batch, int, "GWI_MAX_BATCH")                    /* hyper-parameter points per launch the buffers hold (1..64, default 16) */                             \
  X(deterministic, int, "GWI_DETERMINISTIC")            /* 1: replay mode of the shared gradient rows (one replica per lane) */                                  \
  X(gacc_rep, int, "GWI_GACC_REP")                      /* replicas of the gradient rows in LDS (any count but 16 runs the SAFE instantiation) */                 \
  X(batch_mfma, int, "GWI_BATCH_MFMA")                  /* 0 keeps the 4-tap batched kernel, 1 compiles a missing matrix-core one now, 2 uses it for every batch size */ \
  X(batch_rows, int, "GWI_BATCH_ROWS")                  /* 1: the LDS-row variant of the matrix-core kernel (2: for every batch size) */                         \
  X(batch_autotune, int, "GWI_BATCH_AUTOTUNE")          /* 1: measure the two batched kernels instead of the static rule */                                      \
  X(rows_rep, int, "GWI_ROWS_REP")                      /* sample-slot replicas of the LDS-row variant's gradient rows (1..4) */                                 \
  /* ---- launch geometry (plan_geometry) */                                                                                                                     \
  X(samples_per_block, long long, "GWI_SAMPLES_PER_BLOCK") /* samples per scan workgroup (whole trips); set: no single-round, small-catalog or tile-cap rule */  \
  X(single_round, int, "GWI_SINGLE_ROUND")              /* 0: no sizing of the workgroups for one round of resident ones */                                      \
  X(small_geometry, int, "GWI_SMALL_GEOMETRY")          /* 0: no small-catalog rule (one sample per lane on many small workgroups) */                            \
  X(small_wgs_per_cu, double, "GWI_SMALL_WGS_PER_CU")   /* workgroups per CU the small-catalog rule aims for (default 4, at least 0.5) */                        \
  X(tile_cap, int, "GWI_TILE_CAP")                      /* 0: no cap of 16 tiles per event */                                                                    \
  X(pe_chunk, int, "GWI_PE_CHUNK")                      /* experiment knobs: exact tile sizes (the kernel takes any size) */                                     \
  X(inj_chunk, int, "GWI_INJ_CHUNK")                                                                                                                             \
  X(tiles_per_inj_group, int, "GWI_TILES_PER_INJ_GROUP") /* injection tile records per combine workgroup (1..64, default 16) */                                  \
  X(batch_geometry, int, "GWI_BATCH_GEOMETRY")          /* 0: batched launches on the single evaluation's geometry (set at all: no pbatch geometry) */            \
  /* ---- parametric batches, buffers, tail launches */                                                                                                          \
  X(pbatch, int, "GWI_PBATCH")                          /* 1: parametric batches load every sample once (scan_pbatch_kernel) */                                  \
  X(pbatch_pts, int, "GWI_PBATCH_PTS")                  /* ... points per grid row (naming a row size asks for the rows mode) */                                 \
  X(pbatch_balanced, int, "GWI_PBATCH_BALANCED")        /* ... 0: rows mode instead of evenly dealt (tile, point) units */                                       \
  X(pbatch_wgs_per_cu, int, "GWI_PBATCH_WGS_PER_CU")    /* ... resident workgroups per CU (1..16) instead of the occupancy query */                              \
  X(stage_kernel, int, "GWI_STAGE_KERNEL")              /* 0: upload theta blocks with hipMemcpyAsync instead of the staging kernel */                           \
  X(final_groups, int, "GWI_FINAL_GROUPS")              /* workgroups of the final launch (1..64) */                                                             \
  X(host_final_bytes, long long, "GWI_HOST_FINAL_BYTES") /* most bytes of per-group rows the host sums itself (default 120 KiB) */                               \
  X(host_final, int, "GWI_HOST_FINAL")                  /* 0: the final launch sums whatever the size */                                                         \
  X(combine_threads, int, "GWI_COMBINE_THREADS")        /* workgroup size of the combine launch (64, anything else 256) */

struct Knobs {
#define GWI_X(member, T, name) Knob<T> member;
  GWI_PLAN_KNOBS(GWI_X)
#undef GWI_X
  // read once per gwi_create, never cached: a process may change the variables between engines
  static Knobs from_env() {
    Knobs k;
#define GWI_X(member, T, name) \
  if (const char* e = std::getenv(name)) k.member = {true, parse((T*)nullptr, e)};
    GWI_PLAN_KNOBS(GWI_X)
#undef GWI_X
    return k;
  }

  static int parse(int*, const char* e) { return std::atoi(e); }
  static long long parse(long long*, const char* e) { return std::atoll(e); }
  static double parse(double*, const char* e) { return std::atof(e); }
};

// Explicit geometry knobs switch the small-catalog rule off.
inline bool explicit_geometry(const Knobs& k) { return k.samples_per_block.set || k.pe_chunk.set || k.inj_chunk.set || k.small_geometry.off(); }

// Small catalogs of spline models (fewer than ~11 trips of 256 samples per CU: BASELINE config 3) are a chain of latencies, not
// a throughput problem: more and smaller workgroups of the one-sample-per-lane sibling -- four per CU, equal tiles inside an
// event -- measured 12.5-12.9 us for the config-3 scan against 13.4-14.3 for 443 workgroups of two samples per lane and two trips
// (tools/geometry_sweep.py; profiles/round3/EXPERIMENTS.md).
inline bool small_catalog(long long n_ev, long long n_pe, long long n_inj, int n_cus) {
  const long long total = n_ev * n_pe + n_inj;
  return total < 2816LL * n_cus && total >= 64LL * n_cus;
}

// Tiling of one launch geometry: posterior samples in tiles of chunk_pe per event, injections in tiles of chunk_inj, the
// injection tiles combined in n_inj_groups groups of tiles_per_inj_group records.
struct Geometry {
  int chunk_pe = 0, chunk_inj = 0, tiles_per_event = 0, n_inj_tiles = 0, n_scan_blocks = 0, tiles_per_inj_group = 0, n_inj_groups = 0;
  bool distinct = false;  // the batched geometry only: it exists, fits the tail kernels and differs from the single evaluation's
};

// Tiles and groups of a pair of tile sizes.  Injection tiles are combined in groups of <= tiles_per_inj_group records (16: one
// workgroup each, and a group's tile values are then all requested in the combine kernel's first memory round trip, kEarly
// there; <= 64: one tile per lane in combine_kernel).
inline Geometry tile(long long n_ev, long long n_pe, long long n_inj, int chunk_pe, int chunk_inj, int tiles_per_inj_group) {
  auto packable = [](int c) { return c >= 32768 && c % 256 ? (c / 256 + 1) * 256 : c; };  // (chunk_packs: multiples of 256 from 32 768 on)
  Geometry g;
  g.chunk_pe = packable(chunk_pe);
  g.chunk_inj = packable(chunk_inj);
  g.tiles_per_event = (int)((n_pe + g.chunk_pe - 1) / g.chunk_pe);
  g.n_inj_tiles = (int)((n_inj + g.chunk_inj - 1) / g.chunk_inj);
  g.n_scan_blocks = (int)(n_ev * g.tiles_per_event + g.n_inj_tiles);
  g.tiles_per_inj_group = tiles_per_inj_group;
  g.n_inj_groups = std::max(1, (g.n_inj_tiles + g.tiles_per_inj_group - 1) / g.tiles_per_inj_group);
  if (g.n_inj_groups > 64) {  // final_kernel maps groups to the lanes of one wave
    g.tiles_per_inj_group = (g.n_inj_tiles + 63) / 64;
    g.n_inj_groups = (g.n_inj_tiles + g.tiles_per_inj_group - 1) / g.tiles_per_inj_group;
  }
  return g;
}

// the tail kernels map the tile records of one group to the lanes of ONE wave
inline bool fits_tail(const Geometry& g) { return g.tiles_per_event <= 64 && g.tiles_per_inj_group <= 64 && g.n_inj_groups <= 64; }

struct LaunchPlan {
  Geometry geo[2];  // [0] single evaluations (and batches without a geometry of their own), [1] batched launches where .distinct
};

// The launch geometries of a catalog of n_ev events x n_pe posterior samples and n_inj injections on n_cus CUs, for a scan chain
// of samples_per_lane samples per lane and trip of which scan_occupancy workgroups fit a CU (0: unknown).  small_geometry: the
// small-catalog rule chose this chain; pbatch_spb: samples per workgroup of the one-load-per-sample batched kernel (0: not in use).
// A caller must refuse a plan whose geo[0] does not fits_tail() or whose tile sizes do not chunk_packs().
inline LaunchPlan plan_geometry(long long n_ev, long long n_pe, long long n_inj, int n_cus, int samples_per_lane, int scan_occupancy, bool small_geometry, long long pbatch_spb,
                                const Knobs& knobs) {
  // Default: ~2048 scan workgroups (8 per CU).  A step lasts only ~10 us, so a
  // partial second dispatch round (a few workgroups that can only start when the first finishers
  // retire) costs a large fraction of it: when one round of resident workgroups can hold the whole
  // catalog with <= 4 trips each, size the workgroups for exactly one round instead.
  const long long gran = (long long)samples_per_lane * kBlock;  // every lane carries U samples per trip
  auto round_up = [&](long long v) { return ((v + gran - 1) / gran) * gran; };
  const long long n_pe_pad = round_up(n_pe);
  auto blocks_of = [&](long long cpe, long long cinj) { return n_ev * ((n_pe + cpe - 1) / cpe) + (n_inj + cinj - 1) / cinj; };
  long long spb = knobs.samples_per_block.v, spb_batch = 0;  // spb_batch != 0: batched launches use another tile size
  if (spb <= 0) {
    const long long total = n_ev * n_pe + n_inj;
    spb = (total + 2047) / 2048;
    const bool single_round = !knobs.single_round.off();
    if (single_round && scan_occupancy > 0) {
      const long long capacity = (long long)n_cus * scan_occupancy;
      for (long long cand = gran; cand <= 4 * gran; cand += gran) {
        if (blocks_of(std::min(cand, n_pe_pad), cand) <= capacity) {
          if (cand > spb) spb = cand;
          break;
        }
      }
      // One trip per workgroup where two would still give every CU a workgroup: BATCHED launches take two (geo[1] below).
      // Prologue and record reduction are a quarter of a one-trip workgroup's instructions (config 2, K = 16: scan 52.1 ->
      // 45.3 us, 205 k -> 236 k evals/s); a single evaluation gains nothing from it (16.9 vs 16.8 us) and four concurrent
      // chains lose ~10 %, so the single-evaluation geometry stays at one trip.
      if (spb == gran && blocks_of(std::min(2 * gran, n_pe_pad), 2 * gran) >= (long long)n_cus) spb_batch = 2 * gran;
    }
  }
  spb = std::max(round_up(spb), gran);
  int chunk_pe = (int)std::min(spb, n_pe_pad), chunk_inj = (int)spb;
  if (small_geometry) {
    const long long total = n_ev * n_pe + n_inj;
    double per_cu = 4.0;  // one round of resident workgroups at four waves per SIMD; 2.0 / 2.75 / 3.4 / 4.0 / 5.5 / 7.0 measured 15.4 / 13.8 / 13.7 / 13.1 / 16.2 / 14.7 us on one box
    if (knobs.small_wgs_per_cu.set) per_cu = std::max(0.5, knobs.small_wgs_per_cu.v);
    const long long target = std::max<long long>(64, (long long)((double)total / (per_cu * n_cus) + 0.5));
    const long long tiles_pe = std::max<long long>(1, (n_pe + target / 2) / target);
    chunk_pe = (int)((n_pe + tiles_pe - 1) / tiles_pe);  // equal tiles inside an event
    chunk_inj = (int)target;
    spb_batch = 0;
  }
  // The combine launch requests the records of up to 16 tiles of an event in its first memory round trip (kEarly in
  // combine_group) and needs another dependent round per 16 more: a catalog of few events with many posterior samples each --
  // one rank's share of config 5 on 8 GPUs: 25 events x 10 000 -- got 40 tiles of 256 per event and a 9.5 us combine behind a
  // 10.7 us scan.  At most 16 tiles per event where that still leaves every CU a workgroup: 768-sample tiles there, scan
  // 11.7 us, combine 4.1 us, 27.4 -> 21.3 us per local evaluation (tools/shard_time.py).
  if (!knobs.samples_per_block.set && !knobs.tile_cap.off()) {
    const long long cap_chunk = round_up((n_pe + 15) / 16);
    if (chunk_pe < cap_chunk) {
      const long long inj_chunk = std::max<long long>(chunk_inj, cap_chunk);
      if (blocks_of(cap_chunk, inj_chunk) >= (long long)n_cus) {
        chunk_pe = (int)cap_chunk;
        chunk_inj = (int)inj_chunk;
      }
    }
  }
  // experiment knobs: exact tile sizes (the kernel takes any size; a trip covers samples_per_lane * 256 samples)
  if (knobs.pe_chunk.set) chunk_pe = std::max(1, knobs.pe_chunk.v);
  if (knobs.inj_chunk.set) chunk_inj = std::max(1, knobs.inj_chunk.v);
  // the tail kernels map the tile records of one group to the lanes of ONE wave: an event may have at most 64 tiles, the
  // injections at most 64 groups x 64 tiles.  Few events with very many posterior samples (3 events x 1 M) or a very long
  // injection set exceed that with the default tile size: grow the tiles (whole trips) until they fit.
  chunk_pe = (int)std::max<long long>(chunk_pe, round_up((n_pe + 63) / 64));
  chunk_inj = (int)std::max<long long>(chunk_inj, round_up((n_inj + 64 * 64 - 1) / (64 * 64)));
  LaunchPlan p;
  p.geo[0] = tile(n_ev, n_pe, n_inj, chunk_pe, chunk_inj, knobs.tiles_per_inj_group.set ? std::max(1, std::min(64, knobs.tiles_per_inj_group.v)) : 16);
  if (knobs.batch_geometry.off()) spb_batch = 0;  // batched launches on the single evaluation's geometry
  // parametric batches on scan_pbatch_kernel take single-trip tiles (not distinct below where that is the single geometry)
  if (pbatch_spb > 0 && !knobs.batch_geometry.set) spb_batch = pbatch_spb;
  if (spb_batch > 0 && !knobs.pe_chunk.set && !knobs.inj_chunk.set) {
    Geometry& b = p.geo[1];
    b = tile(n_ev, n_pe, n_inj, (int)std::min(spb_batch, n_pe_pad), (int)spb_batch, 16);
    // within what the tail kernels take (64 tile records per group, 64 groups); the engine's buffers hold either geometry
    b.distinct = fits_tail(b) && b.tiles_per_event < (1 << kGeomTilesBits) && (b.chunk_pe != p.geo[0].chunk_pe || b.chunk_inj != p.geo[0].chunk_inj);
  }
  return p;
}

// Dynamic LDS of the scan kernel: the workgroup's spline-gradient rows, [n_theta][rep] doubles (spline_scatter in
// gwi_device.h).  rep = 64 would give every lane its own replica; 16 (four lanes per replica, bank = replica) measured
// the same or better on the BASELINE catalogs (config 5 scan: rep 8 / 16 / 32 / 64 = 61.5 / 51.2 / 51.7 / 70.0 us, config 3:
// 15.5 / 14.6 / 15.3 / 16.1) because the rows must also fit next to the kernel's static LDS as many times as the
// register budget allows workgroups on a CU, and are zeroed and summed once per workgroup.
struct GaccRows {
  int rep;
  size_t scan_lds;  // bytes: the rows and, behind them, the power-basis table of the spline values (gwi_device.h: spline_poly)
};
inline GaccRows gacc_replicas(int n_theta, size_t static_lds, bool deterministic, const Knobs& knobs) {
  const size_t lds_per_cu = 160 * 1024;  // gfx950: 160 KiB per CU
  // 16 replicas: what the regular scan kernels are compiled for (immediate row offsets).  Where rows that wide cost a
  // resident workgroup (n_theta beyond ~100), that is the cheaper loss: 8 replicas measured 20 % slower at config 5.
  // Any other count (GWI_GACC_REP, the replay mode's 64) runs the SAFE instantiation, which takes it at run time.
  int rep = 1 << kRegularRepShift;
  if (knobs.gacc_rep.set) rep = knobs.gacc_rep.v;
  if (deterministic) rep = 64;  // one replica per lane: a wave instruction never meets itself on an address
  rep = std::max(1, std::min(64, rep));
  while (rep & (rep - 1)) rep &= rep - 1;  // power of two
  const size_t poly_lds = 4 * sizeof(double) * (size_t)kPolyStride;
  while (rep > 1 && sizeof(double) * (size_t)n_theta * rep + poly_lds + static_lds > lds_per_cu) rep >>= 1;
  return {rep, sizeof(double) * (size_t)n_theta * rep + poly_lds};
}

}  // namespace gwi_plan
