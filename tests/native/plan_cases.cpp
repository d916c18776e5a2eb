// plan_cases — the shim's planning code (rt_plan.cpp) on cases read from a file, for a build with
// the host sanitizers (tests/test_plan_cpu.py compiles this file together with rt_plan.cpp and
// rt_host.cpp and runs it as a child process; it is never loaded into Python and never touches the
// GPU).
//
//   plan_cases CASES      one case per line of CASES, one line of output per case:
//
//   pack W H S SPP ROW_BEGIN ROW_END FILE    FILE: the header's floats (rt_header_bytes(S, SPP) bytes)
//        -> pack KEY NCL CLUSTERS MASKS      hex bytes of cull_key, and of pack_header's cluster table
//                                            ([NCL] rows) and masks ([1 + NCL][kClusterWords] u64); "-" = empty
//   order GX GY PER_UNIT NCUR CUR... COST...   NCUR values of the current order, GX*GY*PER_UNIT costs
//        -> order none | order V...
//   slots M PREV NSLOTS PATTERN              PATTERN: M characters, '1' = equals the previous frame's table
//        -> slots BASE SLOT...
//
// Exit 0 = every case ran clean.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../real_time_ray_tracer_amd/csrc/rt_plan.h"

static void hex(const void* p, size_t n) {
  if (n == 0) std::printf(" -");
  else std::printf(" ");
  for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char*)p)[i]);
}

static int pack(std::istringstream& in) {
  rt_config cfg{};
  std::string path;
  in >> cfg.width >> cfg.height >> cfg.num_shapes >> cfg.spp >> cfg.row_begin >> cfg.row_end >> path;
  if (!in) return 2;
  std::vector<float> h(rt_header_bytes(cfg.num_shapes, cfg.spp) / 4);
  std::ifstream f(path, std::ios::binary);
  if (!f.read((char*)h.data(), (std::streamsize)(h.size() * 4))) return 3;
  std::vector<unsigned char> key(rt::cull_key(cfg, h.data(), nullptr, 0));
  if (rt::cull_key(cfg, h.data(), key.data(), key.size()) != key.size()) return 4;
  if (!key.empty()) {  // a key that does not fit is measured, never written
    std::vector<unsigned char> small(key.size() - 1, 0xee);
    if (rt::cull_key(cfg, h.data(), small.data(), small.size()) != key.size()) return 5;
  }
  const int Sc = rt::table_stride(cfg);
  std::vector<rt::Row> tab(rt::table_vec4(Sc, cfg.spp));
  int nobj = -1, np = -1, ncl = -1;
  if (rt::pack_header(cfg, h.data(), tab.data(), nobj, np, ncl) != RT_OK) return 6;
  if (nobj != rt::header_nobj(h.data(), cfg.num_shapes) || np < 0 || ncl < 0 || ncl > rt::kMaxClusters) return 7;
  std::printf("pack");
  hex(key.data(), key.size());
  std::printf(" %d", ncl);
  hex(tab.data() + rt::cluster_table(Sc), (size_t)ncl * sizeof(rt::Row));
  hex(tab.data() + rt::cluster_mask_table(Sc), (size_t)(1 + ncl) * rt::kClusterWords * sizeof(uint64_t));
  std::printf("\n");
  return 0;
}

static int order(std::istringstream& in) {
  int gx = 0, gy = 0, per = 0;
  size_t ncur = 0;
  in >> gx >> gy >> per >> ncur;
  if (!in || gx < 1 || gy < 1 || per < 1) return 2;
  std::vector<unsigned> cur(ncur), cost((size_t)gx * gy * per), next;
  for (auto& v : cur) in >> v;
  for (auto& v : cost) in >> v;
  if (!in) return 3;
  std::printf("order");
  if (!rt::sched_order(gx, gy, per, cost.data(), cur, next)) std::printf(" none");
  else
    for (unsigned v : next) std::printf(" %u", v);
  std::printf("\n");
  return 0;
}

static int slots(std::istringstream& in) {
  int m = 0, prev = 0, nslots = 0;
  std::string pattern;
  in >> m >> prev >> nslots >> pattern;
  if (!in || m < 1 || (int)pattern.size() != m) return 2;
  std::vector<unsigned char> same(m);
  for (int j = 0; j < m; ++j) same[j] = pattern[j] == '1';
  std::vector<int> slot(m, -99);
  std::printf("slots %d", rt::batch_slots(same.data(), m, prev, nslots, slot.data()));
  for (int s : slot) std::printf(" %d", s);
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream cases(argv[1]);
  if (!cases) return 2;
  std::string line;
  for (int n = 1; std::getline(cases, line); ++n) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    const int rc = what == "pack" ? pack(in) : what == "order" ? order(in) : what == "slots" ? slots(in) : 2;
    if (rc != 0) {
      std::fprintf(stderr, "case %d (%s): %d\n", n, what.c_str(), rc);
      return 10 + rc;
    }
  }
  return 0;
}
