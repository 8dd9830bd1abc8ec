// Driver of tests/test_plan_cpu.py: the launch planning of gwi_create (gwinferno_amd/csrc/gwi_plan.h) without an engine.
// One case per line of standard input, one line of integers per case on standard output:
//   G n_ev n_pe n_inj n_cus samples_per_lane scan_occupancy small_geometry pbatch KNOB VALUE
//     -> refused, the seven fields of the single-evaluation geometry, the seven of the batched one, distinct
//   L n_theta static_lds deterministic KNOB VALUE
//     -> rep scan_lds
// KNOB is the one environment variable set for the case ("-": none); it reaches the plan through Knobs::from_env().
#include "gwi_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace gwi_plan;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string tag, knob, value;
    in >> tag;
    if (tag == "G") {
      long long n_ev, n_pe, n_inj;
      int n_cus, u, occ, small, pbatch;
      in >> n_ev >> n_pe >> n_inj >> n_cus >> u >> occ >> small >> pbatch >> knob >> value;
      if (!in) return 2;
      if (knob != "-") setenv(knob.c_str(), value.c_str(), 1);
      const LaunchPlan p = plan_geometry(n_ev, n_pe, n_inj, n_cus, u, occ, small != 0, pbatch ? (long long)u * kBlock : 0, Knobs::from_env());
      if (knob != "-") unsetenv(knob.c_str());
      // what gwi_create refuses: 1 "more than 64 tile records per group", 2 "outside the scan's packed geometry"
      const Geometry &g = p.geo[0], &b = p.geo[1];
      int refused = 0;
      if (!fits_tail(g))
        refused = 1;
      else if (g.tiles_per_event >= (1 << kGeomTilesBits) || !chunk_packs(g.chunk_pe) || !chunk_packs(g.chunk_inj) || (b.distinct && (!chunk_packs(b.chunk_pe) || !chunk_packs(b.chunk_inj))))
        refused = 2;
      std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", refused, g.chunk_pe, g.chunk_inj, g.tiles_per_event, g.n_inj_tiles, g.n_scan_blocks, g.tiles_per_inj_group,
                  g.n_inj_groups, b.chunk_pe, b.chunk_inj, b.tiles_per_event, b.n_inj_tiles, b.n_scan_blocks, b.tiles_per_inj_group, b.n_inj_groups, b.distinct ? 1 : 0);
    } else if (tag == "L") {
      int n_theta, det;
      long long static_lds;
      in >> n_theta >> static_lds >> det >> knob >> value;
      if (!in) return 2;
      if (knob != "-") setenv(knob.c_str(), value.c_str(), 1);
      const GaccRows r = gacc_replicas(n_theta, (size_t)static_lds, det != 0, Knobs::from_env());
      if (knob != "-") unsetenv(knob.c_str());
      std::printf("%d %zu\n", r.rep, r.scan_lds);
    } else if (!tag.empty()) {
      return 2;
    }
  }
  std::puts("OK");
  return 0;
}
