// ray_query_cases — the ray queries' host specification (rt_query_host.cpp) on rays read from a file,
// for a build with the host sanitizers (tests/test_ray_query_cpu.py compiles this file together with
// rt_query_host.cpp and runs it as a child process; it is never loaded into Python and never touches
// the GPU).  Every input and output lives in a heap block of exactly its size, so a read or write
// one element past an end is reported.
//
//   ray_query_cases HEADER S SPP W H RAYS N THR
//     HEADER: the header's floats (rt_header_bytes(S, SPP) bytes); RAYS: N rows of 6 floats (a, b)
//   -> four lines of hex bytes ("-" = empty):
//     trace  T IND NORMALS      rt_trace_rays_host of the rays (a, b) at THR
//     occ    OUT                rt_occluded_host of the segments a -> b
//     pixels ORIGINS DIRS       rt_pixel_rays_host of the pixels (k % 7 - 2, k / 7 - 1), k < N
//     nulls  ok                 the same calls with every output NULL
//
// Exit 0 = every call returned RT_OK and ran clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>

#include "rt/abi.h"

static void hex(const void* p, size_t n) {
  std::printf(n ? " " : " -");
  for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char*)p)[i]);
}

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  rt_config cfg{};
  cfg.num_shapes = std::atoi(argv[2]);
  cfg.spp = std::atoi(argv[3]);
  cfg.width = std::atoi(argv[4]);
  cfg.height = std::atoi(argv[5]);
  const size_t n = (size_t)std::strtoull(argv[7], nullptr, 10);
  const float thr = std::strtof(argv[8], nullptr);
  const size_t hb = rt_header_bytes(cfg.num_shapes, cfg.spp);
  std::unique_ptr<char[]> header(new char[hb]);
  if (!std::ifstream(argv[1], std::ios::binary).read(header.get(), (std::streamsize)hb)) return 3;
  std::unique_ptr<float[]> a(new float[3 * n]), b(new float[3 * n]);
  {
    std::ifstream f(argv[6], std::ios::binary);
    for (size_t k = 0; k < n; ++k)
      if (!f.read((char*)(a.get() + 3 * k), 12) || !f.read((char*)(b.get() + 3 * k), 12)) return 4;
  }
  std::unique_ptr<float[]> t(new float[n]), nrm(new float[3 * n]), po(new float[3 * n]), pd(new float[3 * n]);
  std::unique_ptr<int32_t[]> ind(new int32_t[n]), xy(new int32_t[2 * n]);
  std::unique_ptr<uint8_t[]> occ(new uint8_t[n]);
  for (size_t k = 0; k < n; ++k) {
    xy[2 * k] = (int32_t)(k % 7) - 2;
    xy[2 * k + 1] = (int32_t)(k / 7) - 1;
  }
  if (rt_trace_rays_host(&cfg, header.get(), hb, a.get(), b.get(), n, thr, t.get(), ind.get(), nrm.get()) != RT_OK) return 5;
  if (rt_occluded_host(&cfg, header.get(), hb, a.get(), b.get(), n, occ.get()) != RT_OK) return 6;
  if (rt_pixel_rays_host(&cfg, header.get(), hb, xy.get(), n, po.get(), pd.get()) != RT_OK) return 7;
  std::printf("trace");
  hex(t.get(), 4 * n);
  hex(ind.get(), 4 * n);
  hex(nrm.get(), 12 * n);
  std::printf("\nocc");
  hex(occ.get(), n);
  std::printf("\npixels");
  hex(po.get(), 12 * n);
  hex(pd.get(), 12 * n);
  std::printf("\n");
  if (rt_trace_rays_host(&cfg, header.get(), hb, a.get(), b.get(), n, thr, nullptr, nullptr, nullptr) != RT_OK) return 8;
  if (rt_occluded_host(&cfg, header.get(), hb, a.get(), b.get(), n, nullptr) != RT_OK) return 9;
  if (rt_pixel_rays_host(&cfg, header.get(), hb, xy.get(), n, nullptr, nullptr) != RT_OK) return 10;
  std::printf("nulls ok\n");
  return 0;
}
