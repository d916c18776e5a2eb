// tree_build_time — host cost of one query-tree build (rt_plan build_query_tree) on an rt_scenegen
// scene, std::chrono around the call; host only (profiles/r18_query_tree.txt).
//
//   c++ -O3 -std=c++17 -ffp-contract=off -Iinclude tools/micro/tree_build_time.cpp \
//       real_time_ray_tracer_amd/csrc/rt_plan.cpp real_time_ray_tracer_amd/csrc/rt_host.cpp -o build/tree_build_time
//   build/tree_build_time [spheres = 2048] [repeats = 200]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../real_time_ray_tracer_amd/csrc/rt_plan.h"

int main(int argc, char** argv) {
  const int S = argc > 1 ? std::atoi(argv[1]) : 2048, reps = argc > 2 ? std::atoi(argv[2]) : 200;
  if (S < 1 || reps < 1) return 2;
  rt_config cfg{};
  cfg.width = cfg.height = 1;
  cfg.num_shapes = S;
  cfg.spp = 1;
  std::vector<float> h(rt_header_bytes(S, 1) / 4);
  if (rt_scenegen(h.data(), S, S, 1, 1234, 16.0f / 9.0f) != RT_OK) return 3;
  const int Sc = rt::table_stride(cfg);
  std::vector<rt::Row> tab(rt::table_vec4_rect(Sc, 1));
  int nobj = 0, np = 0, ncl = 0;
  if (rt::pack_header(cfg, h.data(), tab.data(), nobj, np, ncl) != RT_OK) return 4;
  rt::QueryTreeHost t;
  t.reserve(S);
  std::vector<double> us(reps);
  int nodes = 0;
  for (int k = 0; k < reps; ++k) {
    const auto t0 = std::chrono::steady_clock::now();
    nodes = rt::build_query_tree(tab.data() + rt::sphere_table(Sc), nobj, t);
    us[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  std::sort(us.begin(), us.end());
  std::printf("host build of the query tree, %d spheres (kTreeLeaf %d): %d nodes, %d leaves; %.1f us median, %.1f us min of %d builds\n",
              S, rt::kTreeLeaf, nodes, t.n_leaves, us[reps / 2], us[0], reps);
  return 0;
}
