// mesh_cases.cpp — a stand-alone program over real_time_ray_tracer_amd/csrc/rt_mesh_host.cpp (the mesh
// layer's host-only unit, include/rt/mesh.h), built by tests/test_mesh_cpu.py under the host sanitizers
// and run as a child process.  It reads case lines from the file named by argv[1] and prints one line
// per case:
//
//   mesh NV NT VERTS TRIS RAYS KINDS N
//        VERTS: nv*3 float32, TRIS: nt*3 int32, RAYS: origins, dirs, a, b, each N*3 float32, KINDS: N
//        int32 in [0, 8), the kind of each ray (raw files)
//     -> mesh nodes live dead <boxes hex> <links hex> <order hex> same bad_trace bad_occ hits occluded
//                gate_pairs then gate_hits:gate_rejected for each of the 8 kinds
//        the hierarchy's arrays (rt_mesh_bvh_host), whether a second build gave the same bytes, the rays
//        on which this program's own walk over the skip links differs from rt_mesh_trace_rays_host
//        (t, prim, normals, uv, bit for bit) and rt_mesh_occluded_host, how many rays hit and how many
//        segments are occluded, and the gate's cost: over every (ray, live triangle) pair, the hits an
//        ungated binary32 Moeller-Trumbore (written here from the header) accepts with t > 1e-4, and
//        how many of those rt_mesh_tri_eval_host rejects, by the ray's kind.
//   mono SEED COUNT
//     -> mono count violations inner_pass outer_fail
//        box_pass on COUNT seeded pairs of nested boxes (flat boxes, origins on box planes, zero and
//        subnormal direction components): a violation is an inner box that passes in an outer one
//        that fails.
//   args -> args <status codes of the argument checks>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rt/mesh.h"

namespace {

template <class T>
std::vector<T> read_raw(const std::string& path, size_t count) {
  std::vector<T> v(count);
  std::ifstream f(path, std::ios::binary);
  if (count) f.read((char*)v.data(), (std::streamsize)(count * sizeof(T)));
  if (!f) {
    std::fprintf(stderr, "mesh_cases: cannot read %zu values from %s\n", count, path.c_str());
    std::exit(2);
  }
  return v;
}

std::string hex(const void* p, size_t bytes) {
  if (bytes == 0) return "-";
  static const char* d = "0123456789abcdef";
  std::string s(2 * bytes, '0');
  for (size_t i = 0; i < bytes; ++i) {
    s[2 * i] = d[((const unsigned char*)p)[i] >> 4];
    s[2 * i + 1] = d[((const unsigned char*)p)[i] & 15];
  }
  return s;
}

bool same_bits(const float* a, const float* b, int n) { return std::memcmp(a, b, (size_t)n * 4) == 0; }

bool all_finite(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!(std::fabs(p[i]) <= FLT_MAX)) return false;
  return true;
}

struct Tree {
  std::vector<float> boxes;
  std::vector<int32_t> links, order;
  int nodes = 0, live = 0;
};

bool build(const std::vector<float>& verts, int nv, const std::vector<int32_t>& tris, int nt, Tree& t) {
  const int cap = 2 * nt + 1;
  t.boxes.assign(6 * (size_t)cap, 0.0f);
  t.links.assign(3 * (size_t)cap, 0);
  t.order.assign((size_t)nt + 1, 0);
  t.nodes = rt_mesh_bvh_host(verts.data(), nv, tris.data(), nt, t.boxes.data(), t.links.data(), cap, t.order.data(), nt + 1,
                             &t.live);
  if (t.nodes < 0) return false;
  t.boxes.resize(6 * (size_t)t.nodes);
  t.links.resize(3 * (size_t)t.nodes);
  t.order.resize((size_t)t.live);
  return true;
}

// This program's walk: at node k, to k + 1 when the box passes (after the members of a leaf), else to
// skip[k]; candidates merged by (t, index).  The rule itself is asked of the public host functions.
template <class F>
void walk(const Tree& tr, const float* o, const float* d, F member) {
  int k = 0;
  while (k < tr.nodes) {
    const float* box = &tr.boxes[6 * (size_t)k];
    const int32_t* ln = &tr.links[3 * (size_t)k];
    if (rt_mesh_box_pass_host(o, d, box, box + 3)) {
      for (int j = 0; j < ln[2]; ++j)
        if (member(tr.order[(size_t)ln[1] + j])) return;
      k = k + 1;
    } else {
      k = ln[0];
    }
  }
}

void normal_of(const float* v0, const float* v1, const float* v2, float n[3]) {
  const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const float il = 1.0f / std::sqrt(std::fmaf(c[2], c[2], std::fmaf(c[1], c[1], c[0] * c[0])));
  n[0] = c[0] * il, n[1] = c[1] * il, n[2] = c[2] * il;
}

float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
void cross3(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

// Moeller-Trumbore as the header states it, without the box gate
float ungated(const float* o, const float* d, const float* v0, const float* v1, const float* v2) {
  float e1[3], e2[3], s[3], p[3], q[3];
  for (int a = 0; a < 3; ++a) e1[a] = v1[a] - v0[a], e2[a] = v2[a] - v0[a], s[a] = o[a] - v0[a];
  cross3(d, e2, p);
  const float det = dot3(e1, p);
  if (!(det != 0.0f)) return -1.0f;
  const float inv = 1.0f / det;
  const float u = dot3(s, p) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return -1.0f;
  cross3(s, e1, q);
  const float v = dot3(d, q) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return -1.0f;
  return dot3(e2, q) * inv;
}

void mesh_case(std::istringstream& in) {
  int nv, nt;
  size_t n;
  std::string vpath, tpath, rpath, kpath;
  in >> nv >> nt >> vpath >> tpath >> rpath >> kpath >> n;
  const std::vector<float> verts = read_raw<float>(vpath, 3 * (size_t)nv);
  const std::vector<int32_t> tris = read_raw<int32_t>(tpath, 3 * (size_t)nt);
  const std::vector<float> rays = read_raw<float>(rpath, 12 * n);
  const std::vector<int32_t> kinds = read_raw<int32_t>(kpath, n);
  const float *O = rays.data(), *D = O + 3 * n, *A = D + 3 * n, *B = A + 3 * n;
  Tree tr, again;
  if (!build(verts, nv, tris, nt, tr) || !build(verts, nv, tris, nt, again)) {
    std::printf("mesh -1\n");
    return;
  }
  const int same = tr.nodes == again.nodes && tr.boxes == again.boxes && tr.links == again.links && tr.order == again.order;
  auto V = [&](int tri, int c) { return &verts[3 * (size_t)tris[3 * (size_t)tri + c]]; };

  const float thr = 1e-4f;
  std::vector<float> t(n), nrm(3 * n), uv(2 * n);
  std::vector<int32_t> prim(n);
  std::vector<uint8_t> occ(n);
  int rc = rt_mesh_trace_rays_host(verts.data(), nv, tris.data(), nt, O, D, n, 0, thr, t.data(), prim.data(), nrm.data(),
                                   uv.data());
  rc |= rt_mesh_occluded_host(verts.data(), nv, tris.data(), nt, A, B, n, 0, occ.data());
  if (rc != RT_OK) {
    std::printf("mesh -2\n");
    return;
  }
  long bad_trace = 0, bad_occ = 0, hits = 0, occluded = 0;
  for (size_t k = 0; k < n; ++k) {
    const float *o = O + 3 * k, *d = D + 3 * k;
    float bt = -1.0f, buv[2] = {0.0f, 0.0f}, bn[3] = {0.0f, 0.0f, 0.0f};
    int bi = -1;
    if (all_finite(o, 3) && all_finite(d, 3))
      walk(tr, o, d, [&](int i) {
        float w[2];
        const float ti = rt_mesh_tri_eval_host(o, d, V(i, 0), V(i, 1), V(i, 2), w);
        if (ti > thr && (bt < 0.0f || ti < bt || (ti == bt && i < bi))) bt = ti, bi = i, buv[0] = w[0], buv[1] = w[1];
        return false;
      });
    if (bi >= 0) normal_of(V(bi, 0), V(bi, 1), V(bi, 2), bn);
    if (!same_bits(&bt, &t[k], 1) || bi != prim[k] || !same_bits(bn, &nrm[3 * k], 3) || !same_bits(buv, &uv[2 * k], 2))
      ++bad_trace;
    hits += prim[k] >= 0;
    // the segment a -> b
    const float *a = A + 3 * k, *b = B + 3 * k;
    const float lv[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float l2 = dot3(lv, lv);
    const float il = 1.0f / std::sqrt(l2), len = std::sqrt(l2);
    const float l[3] = {lv[0] * il, lv[1] * il, lv[2] * il};
    const float s[3] = {0.01f * l[0], 0.01f * l[1], 0.01f * l[2]};
    const float np[3] = {a[0] + s[0], a[1] + s[1], a[2] + s[2]};
    uint8_t mine = 0;
    if (all_finite(np, 3) && all_finite(l, 3))
      walk(tr, np, l, [&](int i) {
        const double ti = (double)rt_mesh_tri_eval_host(np, l, V(i, 0), V(i, 1), V(i, 2), nullptr);
        if (ti > (double)0.0001f) {
          const double dx = ti * (double)l[0], dy = ti * (double)l[1], dz = ti * (double)l[2];
          if (std::sqrt(std::fma(dz, dz, std::fma(dy, dy, dx * dx))) < (double)len) mine = 1;
        }
        return mine != 0;
      });
    bad_occ += mine != occ[k];
    occluded += occ[k];
  }
  // the gate's cost
  long pairs = 0, gate_hits[8] = {0}, rejected[8] = {0};
  std::vector<int> live;
  for (int i = 0; i < nt; ++i)
    if (all_finite(V(i, 0), 3) && all_finite(V(i, 1), 3) && all_finite(V(i, 2), 3)) live.push_back(i);
  for (size_t k = 0; k < n; ++k) {
    const float *o = O + 3 * k, *d = D + 3 * k;
    if (!all_finite(o, 3) || !all_finite(d, 3)) continue;
    for (int i : live) {
      ++pairs;
      const float tu = ungated(o, d, V(i, 0), V(i, 1), V(i, 2));
      if (!(tu > 1e-4f)) continue;
      ++gate_hits[kinds[k] & 7];
      const float tg = rt_mesh_tri_eval_host(o, d, V(i, 0), V(i, 1), V(i, 2), nullptr);
      if (!same_bits(&tu, &tg, 1)) ++rejected[kinds[k] & 7];
    }
  }
  std::printf("mesh %d %d %d %s %s %s %d %ld %ld %ld %ld %ld", tr.nodes, tr.live, nt - tr.live,
              hex(tr.boxes.data(), tr.boxes.size() * 4).c_str(), hex(tr.links.data(), tr.links.size() * 4).c_str(),
              hex(tr.order.data(), tr.order.size() * 4).c_str(), same, bad_trace, bad_occ, hits, occluded, pairs);
  for (int c = 0; c < 8; ++c) std::printf(" %ld:%ld", gate_hits[c], rejected[c]);
  std::printf("\n");
}

// xorshift64*
struct Rng {
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
  int below(int n) { return (int)(next() >> 33) % n; }
  // a coordinate in [-4, 4]: half of them multiples of 1/4, so equal values are common
  float coord() { return below(2) ? (float)(below(33) - 16) * 0.25f : (float)(unit() * 8.0 - 4.0); }
};

void mono_case(std::istringstream& in) {
  uint64_t seed;
  long count;
  in >> seed >> count;
  Rng g{seed * 0x9E3779B97F4A7C15ull + 1};
  long violations = 0, inner_pass = 0, outer_fail = 0;
  for (long c = 0; c < count; ++c) {
    float ilo[3], ihi[3], olo[3], ohi[3], o[3], d[3], aim[3];
    for (int a = 0; a < 3; ++a) {
      const float p = g.coord(), q = g.below(4) == 0 ? p : g.coord();  // a quarter of the axes flat
      ilo[a] = p < q ? p : q, ihi[a] = p < q ? q : p;
      // the outer box: the same plane, the next float out, or a step away (rounding keeps containment)
      const int kl = g.below(3), kh = g.below(3);
      olo[a] = kl == 0 ? ilo[a] : kl == 1 ? std::nextafterf(ilo[a], -INFINITY) : ilo[a] - (float)g.unit();
      ohi[a] = kh == 0 ? ihi[a] : kh == 1 ? std::nextafterf(ihi[a], INFINITY) : ihi[a] + (float)g.unit();
      const int ko = g.below(6);  // the origin: anywhere, or on one of the four planes
      o[a] = ko == 0 ? ilo[a] : ko == 1 ? ihi[a] : ko == 2 ? olo[a] : ko == 3 ? ohi[a] : g.coord();
      const int ka = g.below(4);  // the aim: a plane of the inner box, or a point of its extent
      aim[a] = ka == 0 ? ilo[a] : ka == 1 ? ihi[a] : ilo[a] + (ihi[a] - ilo[a]) * (float)g.unit();
    }
    for (int a = 0; a < 3; ++a) {
      d[a] = g.below(4) ? aim[a] - o[a] : g.coord();  // mostly aimed at the inner box
      const int kd = g.below(10);
      if (kd == 0) d[a] = 0.0f;
      else if (kd == 1) d[a] = g.below(2) ? 1e-40f : -7e-42f;  // subnormal
      else if (kd == 2) d[a] = -0.0f;
      else if (kd == 3) d[a] *= 1e-30f;
    }
    const int pi = rt_mesh_box_pass_host(o, d, ilo, ihi), po = rt_mesh_box_pass_host(o, d, olo, ohi);
    inner_pass += pi;
    outer_fail += !po;
    violations += pi && !po;
  }
  std::printf("mono %ld %ld %ld %ld\n", count, violations, inner_pass, outer_fail);
}

void args_case() {
  const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, nanv[9] = {0, 0, 0, NAN, 0, 0, 0, 1, 0};
  const int32_t tri[3] = {0, 1, 2}, bad[3] = {0, 1, 3}, neg[3] = {0, -1, 2};
  const float o[3] = {0.25f, 0.25f, 1.0f}, d[3] = {0, 0, -1};
  float t = -1.0f, n3[3], uv[2], boxes[12];
  int32_t prim, links[6], order[2];
  uint8_t oc = 0;
  int live = -1;
  std::printf("args");
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 0, 1e-4f, &t, &prim, n3, uv));        // 0
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 4, 1e-4f, &t, &prim, n3, uv));        // a stray flag
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 0, -1.0f, &t, &prim, n3, uv));        // thr < 0
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 0, NAN, &t, &prim, n3, uv));          // thr NaN
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 0, INFINITY, &t, &prim, n3, uv));     // thr inf
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, nullptr, d, 1, 0, 0.0f, &t, &prim, n3, uv));   // NULL input
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, nullptr, nullptr, 0, 0, 0.0f, 0, 0, 0, 0));    // n = 0: ok
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, bad, 1, o, d, 1, 0, 0.0f, &t, &prim, n3, uv));         // index out of range
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, neg, 1, o, d, 1, 0, 0.0f, &t, &prim, n3, uv));         // negative index
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, RT_MESH_MAX_TRIANGLES + 1, o, d, 1, 0, 0.0f, &t, &prim, n3, uv));
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, RT_MESH_MERGE, 0.0f, nullptr, &prim, n3, uv));  // merge, no t
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, 1, 0, 0.0f, nullptr, nullptr, nullptr, nullptr));  // no output: ok
  std::printf(" %d", rt_mesh_trace_rays_host(v, 3, tri, 1, o, d, ((size_t)1 << 28) + 1, 0, 0.0f, &t, &prim, n3, uv));
  std::printf(" %d", rt_mesh_occluded_host(v, 3, tri, 1, o, d, 1, RT_MESH_ONE_ORIGIN, &oc));              // not a flag here
  std::printf(" %d", rt_mesh_occluded_host(v, 3, tri, 1, o, nullptr, 1, 0, &oc));
  std::printf(" %d", rt_mesh_occluded_host(v, 3, tri, 1, o, d, 1, 0, nullptr));                           // nothing asked: ok
  std::printf(" %d", rt_mesh_occluded_host(v, 3, tri, 1, o, d, 1, RT_MESH_MERGE, nullptr));
  std::printf(" %d", rt_mesh_bvh_host(v, 3, tri, 1, boxes, links, 2, order, 2, &live));                   // 1 node
  std::printf(" %d", rt_mesh_bvh_host(v, 3, tri, 1, boxes, links, 0, order, 2, &live));                   // node_cap too small
  std::printf(" %d", rt_mesh_bvh_host(v, 3, tri, 1, boxes, links, 2, order, 0, &live));                   // leaf_cap too small
  std::printf(" %d", rt_mesh_bvh_host(v, 3, bad, 1, boxes, links, 2, order, 2, &live));
  std::printf(" %d", rt_mesh_bvh_host(nanv, 3, tri, 1, boxes, links, 2, order, 2, &live));                // a dead mesh: 0 nodes
  std::printf(" %d", live);
  std::printf(" %d", rt_mesh_box_pass_host(o, d, nullptr, v));
  std::printf(" %g", rt_mesh_tri_eval_host(o, d, v, v + 3, nullptr, uv));
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "mesh") mesh_case(in);
    else if (what == "mono") mono_case(in);
    else if (what == "args") args_case();
    else return 2;
  }
  return 0;
}
