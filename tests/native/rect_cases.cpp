// rect_cases — the rectangle rule's host specification (rt_query_host.cpp) and the packing of
// rectangles into the device table (rt_plan.cpp) on a header and rays read from files, for a build
// with the host sanitizers (tests/test_rectangles_cpu.py compiles this file together with
// rt_query_host.cpp, rt_plan.cpp and rt_host.cpp and runs it as a child process; it is never loaded
// into Python and never touches the GPU).  Every input and output lives in a heap block of exactly
// its size, so a read or write one element past an end is reported.
//
//   rect_cases HEADER S SPP RAYS N THR
//     HEADER: the header's floats (rt_header_bytes(S, SPP) bytes); RAYS: N rows of 6 floats (a, b)
//   -> lines of hex bytes ("-" = empty):
//     trace  T IND NORMALS      rt_trace_rays_host_ex of the rays (a, b) at THR, RT_SCENE_RECTANGLES
//     occ    OUT                rt_occluded_host_ex of the segments a -> b, RT_SCENE_RECTANGLES
//     eval   ROW T              rt_rectangle_eval_host of the header's first row of id 3 (ROW, -1: none)
//     pack0  NP TABLE           pack_header without flags: rt::table_vec4 rows (an exact-size block)
//     pack0x NP NR TABLE        pack_header with flags = 0 into the same size
//     pack1  NP NR TABLE        pack_header with RT_SCENE_RECTANGLES: rt::table_vec4_rect rows
//     nulls  ok                 the traced calls with every output NULL
//
// Exit 0 = every call returned RT_OK and ran clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>

#include "../../real_time_ray_tracer_amd/csrc/rt_plan.h"

static void hex(const void* p, size_t n) {
  std::printf(n ? " " : " -");
  for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char*)p)[i]);
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  rt_config cfg{};
  cfg.num_shapes = std::atoi(argv[2]);
  cfg.spp = std::atoi(argv[3]);
  cfg.width = 40;
  cfg.height = 30;
  cfg.row_end = 30;
  const size_t n = (size_t)std::strtoull(argv[5], nullptr, 10);
  const float thr = std::strtof(argv[6], nullptr);
  const size_t hb = rt_header_bytes(cfg.num_shapes, cfg.spp);
  std::unique_ptr<float[]> header(new float[hb / 4]);
  if (!std::ifstream(argv[1], std::ios::binary).read((char*)header.get(), (std::streamsize)hb)) return 3;
  std::unique_ptr<float[]> a(new float[3 * n]), b(new float[3 * n]);
  {
    std::ifstream f(argv[4], std::ios::binary);
    for (size_t k = 0; k < n; ++k)
      if (!f.read((char*)(a.get() + 3 * k), 12) || !f.read((char*)(b.get() + 3 * k), 12)) return 4;
  }
  std::unique_ptr<float[]> t(new float[n]), nrm(new float[3 * n]), te(new float[n]);
  std::unique_ptr<int32_t[]> ind(new int32_t[n]);
  std::unique_ptr<uint8_t[]> occ(new uint8_t[n]);
  const int R = RT_SCENE_RECTANGLES;
  if (rt_trace_rays_host_ex(&cfg, header.get(), hb, a.get(), b.get(), n, thr, R, t.get(), ind.get(), nrm.get()) != RT_OK)
    return 5;
  if (rt_occluded_host_ex(&cfg, header.get(), hb, a.get(), b.get(), n, R, occ.get()) != RT_OK) return 6;
  std::printf("trace");
  hex(t.get(), 4 * n);
  hex(ind.get(), 4 * n);
  hex(nrm.get(), 12 * n);
  std::printf("\nocc");
  hex(occ.get(), n);
  int row = -1;
  for (int i = 0; i < cfg.num_shapes && row < 0; ++i)
    if (header[rt_off_shapes() / 4 + (size_t)i * 20 + 19] == (float)RT_SHAPE_RECTANGLE) row = i;
  if (row >= 0) {
    // the row in a block of its own 20 floats
    std::unique_ptr<float[]> sh(new float[20]);
    for (int k = 0; k < 20; ++k) sh[k] = header[rt_off_shapes() / 4 + (size_t)row * 20 + k];
    for (size_t k = 0; k < n; ++k) te[k] = rt_rectangle_eval_host(sh.get(), a.get() + 3 * k, b.get() + 3 * k);
  }
  std::printf("\neval %d", row);
  hex(te.get(), row >= 0 ? 4 * n : 0);
  const int Sc = rt::table_stride(cfg);
  {
    const size_t rows = rt::table_vec4(Sc, cfg.spp);
    std::unique_ptr<rt::Row[]> tab(new rt::Row[rows]());
    int nobj = -1, np = -1, ncl = -1, nr = -1;
    if (rt::pack_header(cfg, header.get(), tab.get(), nobj, np, ncl) != RT_OK) return 7;
    std::printf("\npack0 %d", np);
    hex(tab.get(), rows * sizeof(rt::Row));
    std::unique_ptr<rt::Row[]> tab2(new rt::Row[rows]());
    if (rt::pack_header(cfg, header.get(), tab2.get(), nobj, np, ncl, 0, nr) != RT_OK) return 8;
    std::printf("\npack0x %d %d", np, nr);
    hex(tab2.get(), rows * sizeof(rt::Row));
  }
  {
    const size_t rows = rt::table_vec4_rect(Sc, cfg.spp);
    std::unique_ptr<rt::Row[]> tab(new rt::Row[rows]());
    int nobj = -1, np = -1, ncl = -1, nr = -1;
    if (rt::pack_header(cfg, header.get(), tab.get(), nobj, np, ncl, R, nr) != RT_OK) return 9;
    std::printf("\npack1 %d %d", np, nr);
    hex(tab.get(), rows * sizeof(rt::Row));
  }
  std::printf("\n");
  if (rt_trace_rays_host_ex(&cfg, header.get(), hb, a.get(), b.get(), n, thr, R, nullptr, nullptr, nullptr) != RT_OK) return 10;
  if (rt_occluded_host_ex(&cfg, header.get(), hb, a.get(), b.get(), n, R, nullptr) != RT_OK) return 11;
  std::printf("nulls ok\n");
  return 0;
}
