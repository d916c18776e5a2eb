// tree_cases — the ray queries' tree (rt_plan.cpp build_query_tree behind rt_query_tree_host) on
// headers read from files, for a build with the host sanitizers (tests/test_query_tree_cpu.py
// compiles this file together with rt_plan.cpp, rt_host.cpp and rt_query_host.cpp and runs it as a
// child process; it is never loaded into Python and never touches the GPU).
//
//   tree_cases CASES      one case per line of CASES, one line of output per case:
//
//   tree S SPP FLAGS FILE     FILE: the header's floats (rt_header_bytes(S, SPP) bytes)
//     -> tree N E A BALLS LINKS ROWS INDEX ALWAYS SAME BAD RAYS
//        N nodes, E leaf entries, A always entries and the five arrays as hex bytes ("-" = empty);
//        SAME: 1 when a second call wrote the same bytes;  BAD: of RAYS random unit rays, those whose
//        (t, ind) by the plain traversal below differ from rt_trace_rays_host_ex's at threshold 0.
//   args                      -> args R1 R2 R3 R4: rt_query_tree_host on a short header, with a stray
//                                flag bit, with too small a node / leaf capacity (each must be -1)
//
// The traversal restates, in plain C, what the kernels do, from the arrays alone: the skip links, a
// ball test in binary64 without margins (a ray misses a ball when its line passes the centre
// farther than R, or when the ball lies behind an origin outside it), rt_trace_rays_host_ex's sphere
// rule for the members and the always list, and the (t, index) merge; the shapes that are no spheres
// come from rt_trace_rays_host_ex itself on a copy of the header whose spheres are blanked.
//
// Exit 0 = every case ran clean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/rt/abi.h"

static void hex(const void* p, size_t n) {
  if (n == 0) std::printf(" -");
  else std::printf(" ");
  for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char*)p)[i]);
}

struct Tree {
  int n = 0, e = 0, a = 0;
  std::vector<float> balls, rows;
  std::vector<int32_t> links, index, always;
};

static int build(const rt_config& cfg, const std::vector<float>& h, int flags, Tree& t) {
  const int S = cfg.num_shapes > 0 ? cfg.num_shapes : 1;
  t.balls.assign((size_t)8 * S, 0.0f);
  t.links.assign((size_t)8 * S, 0);
  t.rows.assign((size_t)4 * S, 0.0f);
  t.index.assign(S, 0);
  t.always.assign(S, 0);
  t.n = rt_query_tree_host(&cfg, h.data(), h.size() * 4, flags, t.balls.data(), t.links.data(), 2 * S, t.rows.data(),
                           t.index.data(), S, t.always.data(), S, &t.e, &t.a);
  return t.n;
}

// rt_trace_rays_host_ex's sphere rule (sphere_eval_ray): binary32, the fused chains written as fmaf
static float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
static float sphere_eval(const float* o, const float* d, const float* g) {
  const float pmc[3] = {o[0] - g[0], o[1] - g[1], o[2] - g[2]};
  const float b = dot3(d, pmc);
  const float del = std::fmaf(g[3], g[3], std::fmaf(b, b, -dot3(pmc, pmc)));
  if (del < 0.0f) return -1.0f;
  if (del == 0.0f) return -1.0f * b;
  const float s = std::sqrt(del);
  const float t1 = -1.0f * b + s, t2 = -1.0f * b - s;
  if (t2 < 0.0f) return t1 < 0.0f ? -1.0f : t1;
  return t2;
}
static void merge(float res, int i, float thr, float& t, int& ind) {
  if (res > thr && (t < 0.0f || res < t || (res == t && i < ind))) t = res, ind = i;
}
// binary64, no margins: the ray (o, d), |d| = 1, cannot meet the ball
static bool ball_missed(const float* o, const float* d, const float* cb) {
  const double v[3] = {(double)cb[0] - o[0], (double)cb[1] - o[1], (double)cb[2] - o[2]};
  const double L2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], b = v[0] * d[0] + v[1] * d[1] + v[2] * d[2];
  const double R = cb[3];
  if (!(R == R) || !(L2 == L2) || !(b == b)) return false;
  return L2 - b * b > R * R || (b < 0.0 && L2 > R * R);
}

// int(simple_shapes[i][4].w), 0 for a value no int holds (as the table's packing)
static int shape_id(const float* shapes, int i) {
  const float idf = shapes[(size_t)i * 20 + 19];
  return (idf > -2147483648.0f && idf < 2147483648.0f) ? (int)idf : 0;
}

static uint64_t rng_state = 0;
static double uni() {  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static int tree(std::istringstream& in) {
  rt_config cfg{};
  int flags = 0;
  std::string path;
  in >> cfg.num_shapes >> cfg.spp >> flags >> path;
  if (!in) return 2;
  cfg.width = cfg.height = 1;
  std::vector<float> h(rt_header_bytes(cfg.num_shapes, cfg.spp) / 4);
  std::ifstream f(path, std::ios::binary);
  if (!f.read((char*)h.data(), (std::streamsize)(h.size() * 4))) return 3;
  Tree t, u;
  if (build(cfg, h, flags, t) < 0) return 4;
  if (build(cfg, h, flags, u) != t.n) return 5;
  const bool same = u.e == t.e && u.a == t.a && u.balls == t.balls && u.links == t.links && u.rows == t.rows &&
                    u.index == t.index && u.always == t.always;
  // the traversal against the linear scan
  const int R = 4096;
  const int S = cfg.num_shapes;
  const float* shapes = h.data() + rt_off_shapes() / 4;
  const int nobj = (int)h[RT_HDR_MODE * 4 + 2];
  std::vector<float> o((size_t)3 * R), d((size_t)3 * R), t_lin(R), t_rest(R);
  std::vector<int32_t> i_lin(R), i_rest(R);
  rng_state = 12345;
  for (int k = 0; k < R; ++k) {
    // origins around and inside the scene (every fourth at a sphere's centre, when there is one)
    for (int c = 0; c < 3; ++c) o[3 * k + c] = (float)(-16.0 + 32.0 * uni());
    if (k % 4 == 0 && nobj > 0) {
      const float* g = shapes + (size_t)((int)(uni() * nobj) % nobj) * 20;
      if (std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]))
        for (int c = 0; c < 3; ++c) o[3 * k + c] = g[c];
    }
    float v[3], s;
    do {
      for (int c = 0; c < 3; ++c) v[c] = (float)(2.0 * uni() - 1.0);
      s = dot3(v, v);
    } while (!(s > 1e-3f && s <= 1.0f));
    const float il = 1.0f / std::sqrt(s);
    for (int c = 0; c < 3; ++c) d[3 * k + c] = v[c] * il;
  }
  if (rt_trace_rays_host_ex(&cfg, h.data(), h.size() * 4, o.data(), d.data(), R, 0.0f, flags, t_lin.data(), i_lin.data(),
                            nullptr) != RT_OK)
    return 6;
  std::vector<float> rest = h;  // the shapes that are no spheres: the spheres' ids blanked
  for (int i = 0; i < S; ++i)
    if (shape_id(shapes, i) == RT_SHAPE_SPHERE) rest[rt_off_shapes() / 4 + (size_t)i * 20 + 19] = 0.0f;
  if (rt_trace_rays_host_ex(&cfg, rest.data(), rest.size() * 4, o.data(), d.data(), R, 0.0f, flags, t_rest.data(),
                            i_rest.data(), nullptr) != RT_OK)
    return 7;
  int bad = 0;
  for (int k = 0; k < R; ++k) {
    float tt = -1.0f;
    int ind = -1;
    if (t.n == 0) {  // no tree: every sphere
      for (int i = 0; i < nobj; ++i)
        if (shape_id(shapes, i) == RT_SHAPE_SPHERE) merge(sphere_eval(&o[3 * k], &d[3 * k], shapes + (size_t)i * 20), i, 0.0f, tt, ind);
    } else {
      for (int j = 0; j < t.a; ++j) merge(sphere_eval(&o[3 * k], &d[3 * k], shapes + (size_t)t.always[j] * 20), t.always[j], 0.0f, tt, ind);
      for (int n = 0; n < t.n;) {
        if (ball_missed(&o[3 * k], &d[3 * k], &t.balls[4 * n])) {
          n = t.links[4 * n];
          continue;
        }
        const int first = t.links[4 * n + 1], count = t.links[4 * n + 2];
        for (int j = first; j < first + count; ++j) merge(sphere_eval(&o[3 * k], &d[3 * k], &t.rows[4 * j]), t.index[j], 0.0f, tt, ind);
        n = n + 1;
      }
    }
    merge(t_rest[k], i_rest[k], 0.0f, tt, ind);
    uint32_t x, y;
    std::memcpy(&x, &tt, 4);
    std::memcpy(&y, &t_lin[k], 4);
    bad += x != y || ind != i_lin[k];
  }
  std::printf("tree %d %d %d", t.n, t.e, t.a);
  hex(t.balls.data(), (size_t)t.n * 16);
  hex(t.links.data(), (size_t)t.n * 16);
  hex(t.rows.data(), (size_t)t.e * 16);
  hex(t.index.data(), (size_t)t.e * 4);
  hex(t.always.data(), (size_t)t.a * 4);
  std::printf(" %d %d %d\n", same ? 1 : 0, bad, R);
  return 0;
}

static int args() {
  rt_config cfg{};
  cfg.width = cfg.height = 1;
  cfg.num_shapes = 64;
  cfg.spp = 4;
  std::vector<float> h(rt_header_bytes(64, 4) / 4);
  if (rt_scenegen(h.data(), 64, 64, 4, 1234, 4.0f / 3.0f) != RT_OK) return 3;
  Tree t;
  if (build(cfg, h, 0, t) <= 0) return 4;
  const int n = t.n, e = t.e;
  auto call = [&](size_t bytes, int flags, int node_cap, int leaf_cap) {
    return rt_query_tree_host(&cfg, h.data(), bytes, flags, t.balls.data(), t.links.data(), node_cap, t.rows.data(),
                              t.index.data(), leaf_cap, t.always.data(), 64, nullptr, nullptr);
  };
  std::printf("args %d %d %d %d\n", call(h.size() * 4 - 4, 0, 128, 64), call(h.size() * 4, 2, 128, 64),
              call(h.size() * 4, 0, n - 1, 64), call(h.size() * 4, 0, 128, e - 1));
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
    const int rc = what == "tree" ? tree(in) : what == "args" ? args() : 2;
    if (rc != 0) {
      std::fprintf(stderr, "case %d (%s): %d\n", n, what.c_str(), rc);
      return 10 + rc;
    }
  }
  return 0;
}
