// rt_mesh_host.cpp — the mesh layer's host-only unit (include/rt/mesh.h): the rule's specification
// (rt_mesh_tri_eval_host, rt_mesh_box_pass_host), the brute-force queries, the hierarchy's build and
// the OBJ reader.  No HIP header; built with -ffp-contract=off like rt_plan.cpp.  The arithmetic is
// rt_mesh_rule.h's.
#include "rt_mesh_host.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/rt/mesh.h"
#include "rt_mesh_rule.h"

namespace rt {
namespace mesh {

namespace {

V3 vert(const float* verts, int i) { return V3{verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2]}; }
V3 at(const float* p, size_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

bool tri_live(const float* verts, const int32_t* tri) {
  return finite(vert(verts, tri[0])) && finite(vert(verts, tri[1])) && finite(vert(verts, tri[2]));
}

bool thr_ok(float thr) { return thr >= 0.0f && thr <= FLT_MAX; }  // finite and >= 0; NaN fails

struct Builder {
  const float* verts;
  const int32_t* tris;
  std::vector<float> key;  // [nt][3]: (v0 + v1) + v2 per component
  Bvh* b;

  void tri_box(int i, V3& lo, V3& hi) const {
    const V3 v0 = vert(verts, tris[3 * (size_t)i]), v1 = vert(verts, tris[3 * (size_t)i + 1]),
             v2 = vert(verts, tris[3 * (size_t)i + 2]);
    lo = mn(mn(v0, v1), v2);
    hi = mx(mx(v0, v1), v2);
  }

  void set_box(int k, V3 lo, V3 hi) {
    float* p = &b->boxes[6 * (size_t)k];
    p[0] = lo.x, p[1] = lo.y, p[2] = lo.z, p[3] = hi.x, p[4] = hi.y, p[5] = hi.z;
  }

  // the subtree over order[lo, hi) in preorder; returns its node
  int node(int begin, int end, bool root) {
    const int k = b->nodes++;
    b->boxes.resize(6 * (size_t)b->nodes);
    b->links.resize(3 * (size_t)b->nodes);
    const int m = end - begin;
    int32_t* ord = b->order.data();
    if (m <= RT_MESH_LEAF || (root && m < RT_MESH_SINGLE_LEAF)) {
      std::sort(ord + begin, ord + end);
      V3 lo, hi;
      tri_box(ord[begin], lo, hi);
      for (int j = begin + 1; j < end; ++j) {
        V3 l2, h2;
        tri_box(ord[j], l2, h2);
        lo = mn(lo, l2);
        hi = mx(hi, h2);
      }
      set_box(k, lo, hi);
      b->links[3 * (size_t)k] = k + 1;
      b->links[3 * (size_t)k + 1] = begin;
      b->links[3 * (size_t)k + 2] = m;
      ++b->leaves;
      return k;
    }
    // the widest axis of the keys' bounds; a NaN extent (inf - inf) is never the widest
    float kmin[3], kmax[3];
    for (int a = 0; a < 3; ++a) kmin[a] = kmax[a] = key[3 * (size_t)ord[begin] + a];
    for (int j = begin + 1; j < end; ++j)
      for (int a = 0; a < 3; ++a) {
        const float c = key[3 * (size_t)ord[j] + a];
        kmin[a] = mn(kmin[a], c);
        kmax[a] = mx(kmax[a], c);
      }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
      if (kmax[a] - kmin[a] > kmax[axis] - kmin[axis]) axis = a;
    // the median cut of the order (key, index): a total order (no key is NaN), so the two halves are
    // the same sets however the selection works
    const int mid = begin + m / 2;
    std::nth_element(ord + begin, ord + mid, ord + end, [&](int32_t x, int32_t y) {
      const float kx = key[3 * (size_t)x + axis], ky = key[3 * (size_t)y + axis];
      return kx < ky || (kx == ky && x < y);
    });
    const int left = node(begin, mid, false);
    const int right = node(mid, end, false);
    const float* bl = &b->boxes[6 * (size_t)left];
    const float* br = &b->boxes[6 * (size_t)right];
    set_box(k, mn(V3{bl[0], bl[1], bl[2]}, V3{br[0], br[1], br[2]}), mx(V3{bl[3], bl[4], bl[5]}, V3{br[3], br[4], br[5]}));
    b->links[3 * (size_t)k] = b->nodes;
    b->links[3 * (size_t)k + 1] = 0;
    b->links[3 * (size_t)k + 2] = 0;
    return k;
  }
};

int check_query(size_t n, int flags, int allowed) {
  if ((flags & ~allowed) != 0 || n > RT_QUERY_MAX_RAYS) return RT_E_INVAL;
  return RT_OK;
}

}  // namespace

int check_mesh(const float* verts, int nv, const int32_t* tris, int nt) {
  if (nv < 0 || nt < 0 || nt > RT_MESH_MAX_TRIANGLES) return RT_E_INVAL;
  if (nt > 0 && (!tris || !verts)) return RT_E_INVAL;
  for (size_t j = 0; j < 3 * (size_t)nt; ++j)
    if (tris[j] < 0 || tris[j] >= nv) return RT_E_INVAL;
  return RT_OK;
}

void build_bvh(const float* verts, const int32_t* tris, int nt, Bvh& out) {
  out = Bvh{};
  Builder bd{verts, tris, {}, &out};
  bd.key.resize(3 * (size_t)nt);
  for (int i = 0; i < nt; ++i) {
    if (!tri_live(verts, tris + 3 * (size_t)i)) {
      ++out.dead;
      continue;
    }
    const V3 v0 = vert(verts, tris[3 * (size_t)i]), v1 = vert(verts, tris[3 * (size_t)i + 1]),
             v2 = vert(verts, tris[3 * (size_t)i + 2]);
    bd.key[3 * (size_t)i] = (v0.x + v1.x) + v2.x;
    bd.key[3 * (size_t)i + 1] = (v0.y + v1.y) + v2.y;
    bd.key[3 * (size_t)i + 2] = (v0.z + v1.z) + v2.z;
    out.order.push_back(i);
  }
  if (!out.order.empty()) bd.node(0, (int)out.order.size(), true);
}

bool bvh_valid(const Bvh& b) {
  const size_t live = b.order.size();
  if (b.nodes < 0 || b.boxes.size() != 6 * (size_t)b.nodes || b.links.size() != 3 * (size_t)b.nodes) return false;
  for (int k = 0; k < b.nodes; ++k) {
    const int32_t skip = b.links[3 * (size_t)k], first = b.links[3 * (size_t)k + 1], count = b.links[3 * (size_t)k + 2];
    if (skip <= k || skip > b.nodes) return false;
    if (count < 0 || count > 15 || first < 0 || (size_t)first + (size_t)count > live) return false;
  }
  return true;
}

void pack_tables(const float* verts, const int32_t* tris, const Bvh& b, std::vector<float>& nodes,
                 std::vector<float>& leaf_tris) {
  nodes.assign(8 * (size_t)b.nodes, 0.0f);
  for (int k = 0; k < b.nodes; ++k) {
    float* p = &nodes[8 * (size_t)k];
    const float* box = &b.boxes[6 * (size_t)k];
    const int32_t skip = b.links[3 * (size_t)k], fc = b.links[3 * (size_t)k + 1] * 16 + b.links[3 * (size_t)k + 2];
    p[0] = box[0], p[1] = box[1], p[2] = box[2];
    std::memcpy(p + 3, &skip, 4);
    p[4] = box[3], p[5] = box[4], p[6] = box[5];
    std::memcpy(p + 7, &fc, 4);
  }
  leaf_tris.assign(12 * b.order.size(), 0.0f);
  for (size_t e = 0; e < b.order.size(); ++e) {
    float* p = &leaf_tris[12 * e];
    const int32_t i = b.order[e];
    for (int c = 0; c < 3; ++c) {
      const V3 v = vert(verts, tris[3 * (size_t)i + c]);
      p[4 * c] = v.x, p[4 * c + 1] = v.y, p[4 * c + 2] = v.z;
    }
    std::memcpy(p + 3, &i, 4);
  }
}

}  // namespace mesh
}  // namespace rt

using namespace rt::mesh;

extern "C" {

float rt_mesh_tri_eval_host(const float o[3], const float d[3], const float v0[3], const float v1[3],
                            const float v2[3], float uv[2]) {
  if (uv) uv[0] = uv[1] = 0.0f;
  if (!o || !d || !v0 || !v1 || !v2) return -1.0f;
  const Hit h = tri_eval(make_ray(at(o, 0), at(d, 0)), at(v0, 0), at(v1, 0), at(v2, 0));
  if (uv && h.t != -1.0f) uv[0] = h.u, uv[1] = h.v;
  return h.t;
}

int rt_mesh_box_pass_host(const float o[3], const float d[3], const float lo[3], const float hi[3]) {
  if (!o || !d || !lo || !hi) return 0;
  return box_pass(make_ray(at(o, 0), at(d, 0)), at(lo, 0), at(hi, 0)) ? 1 : 0;
}

int rt_mesh_trace_rays_host(const float* verts, int nv, const int32_t* tris, int nt, const float* origins,
                            const float* dirs, size_t n, int flags, float thr, float* t_out, int32_t* prim_out,
                            float* normals, float* uv) {
  int rc = check_mesh(verts, nv, tris, nt);
  if (rc != RT_OK) return rc;
  rc = check_query(n, flags, RT_MESH_ONE_ORIGIN | RT_MESH_MERGE);
  if (rc != RT_OK || !thr_ok(thr)) return RT_E_INVAL;
  if (n == 0) return RT_OK;
  if (!origins || !dirs || ((flags & RT_MESH_MERGE) && !t_out)) return RT_E_INVAL;
  std::vector<unsigned char> live((size_t)nt);
  for (int i = 0; i < nt; ++i) live[i] = tri_live(verts, tris + 3 * (size_t)i);
  for (size_t k = 0; k < n; ++k) {
    const Ray r = make_ray(at(origins, (flags & RT_MESH_ONE_ORIGIN) ? 0 : k), at(dirs, k));
    Hit best{-1.0f, 0.0f, 0.0f};
    int prim = -1;
    if (r.ok)
      for (int i = 0; i < nt; ++i) {
        if (!live[i]) continue;
        const int32_t* tr = tris + 3 * (size_t)i;
        const Hit h = tri_eval(r, vert(verts, tr[0]), vert(verts, tr[1]), vert(verts, tr[2]));
        if (h.t > thr && (h.t < best.t || best.t < 0.0f)) {
          best = h;
          prim = i;
        }
      }
    V3 nn{0.0f, 0.0f, 0.0f};
    if (prim >= 0) {
      const int32_t* tr = tris + 3 * (size_t)prim;
      nn = tri_normal(vert(verts, tr[0]), vert(verts, tr[1]), vert(verts, tr[2]));
    }
    if ((flags & RT_MESH_MERGE) && !merge_takes(best.t, prim, t_out[k])) {  // the existing answer stands
      if (prim_out) prim_out[k] = -1;
      if (uv) uv[2 * k] = uv[2 * k + 1] = 0.0f;
      continue;
    }
    if (t_out) t_out[k] = best.t;
    if (prim_out) prim_out[k] = prim;
    if (normals) normals[3 * k] = nn.x, normals[3 * k + 1] = nn.y, normals[3 * k + 2] = nn.z;
    if (uv) uv[2 * k] = best.u, uv[2 * k + 1] = best.v;
  }
  return RT_OK;
}

int rt_mesh_occluded_host(const float* verts, int nv, const int32_t* tris, int nt, const float* from,
                          const float* to, size_t n, int flags, uint8_t* out) {
  int rc = check_mesh(verts, nv, tris, nt);
  if (rc != RT_OK) return rc;
  rc = check_query(n, flags, RT_MESH_MERGE);
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  if (!from || !to) return RT_E_INVAL;
  if (!out) return (flags & RT_MESH_MERGE) ? RT_E_INVAL : RT_OK;
  std::vector<unsigned char> live((size_t)nt);
  for (int i = 0; i < nt; ++i) live[i] = tri_live(verts, tris + 3 * (size_t)i);
  for (size_t k = 0; k < n; ++k) {
    float len;
    const Ray r = segment_ray(at(from, k), at(to, k), len);
    uint8_t occ = 0;
    if (r.ok)
      for (int i = 0; i < nt && !occ; ++i) {
        if (!live[i]) continue;
        const int32_t* tr = tris + 3 * (size_t)i;
        const Hit h = tri_eval(r, vert(verts, tr[0]), vert(verts, tr[1]), vert(verts, tr[2]));
        if (occludes(h.t, r.d, (double)len)) occ = 1;
      }
    out[k] = (flags & RT_MESH_MERGE) ? (uint8_t)((out[k] != 0) | occ) : occ;
  }
  return RT_OK;
}

int rt_mesh_bvh_host(const float* verts, int nv, const int32_t* tris, int nt, float* boxes, int32_t* links,
                     int node_cap, int32_t* leaf_index, int leaf_cap, int* live) {
  if (check_mesh(verts, nv, tris, nt) != RT_OK || node_cap < 0 || leaf_cap < 0) return -1;
  Bvh b;
  build_bvh(verts, tris, nt, b);
  if (!bvh_valid(b) || b.nodes > node_cap || b.order.size() > (size_t)leaf_cap) return -1;
  if ((b.nodes > 0 && (!boxes || !links)) || (!b.order.empty() && !leaf_index)) return -1;
  if (b.nodes > 0) {
    std::memcpy(boxes, b.boxes.data(), b.boxes.size() * sizeof(float));
    std::memcpy(links, b.links.data(), b.links.size() * sizeof(int32_t));
    std::memcpy(leaf_index, b.order.data(), b.order.size() * sizeof(int32_t));
  }
  if (live) *live = (int)b.order.size();
  return b.nodes;
}

}  // extern "C"

// ---- OBJ ------------------------------------------------------------------------------------------
namespace {

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// an optional sign and 1 to 10 digits at p; advances p
bool parse_int(const char*& p, const char* end, long long& v) {
  const char* q = p;
  bool neg = false;
  if (q < end && (*q == '-' || *q == '+')) neg = *q++ == '-';
  const char* digits = q;
  long long x = 0;
  while (q < end && *q >= '0' && *q <= '9' && q - digits < 11) x = x * 10 + (*q++ - '0');
  if (q == digits || q - digits > 10) return false;
  v = neg ? -x : x;
  p = q;
  return true;
}

// one vertex of an f statement, [p, end): i, i/j, i/j/k or i//k; the position index i in *index
bool parse_face_vertex(const char* p, const char* end, long long& index) {
  long long other;
  if (!parse_int(p, end, index)) return false;
  if (p == end) return true;
  if (*p++ != '/') return false;
  if (p < end && *p == '/') {  // i//k
    ++p;
    return parse_int(p, end, other) && p == end;
  }
  if (!parse_int(p, end, other)) return false;  // i/j
  if (p == end) return true;
  if (*p++ != '/') return false;  // i/j/k
  return parse_int(p, end, other) && p == end;
}

}  // namespace

extern "C" int rt_obj_parse(const char* text, size_t bytes, float* verts, int vcap, int32_t* tris, int tcap, int* nv_out,
                            int* nt_out, int* err_line) {
  if (err_line) *err_line = 0;
  if (nv_out) *nv_out = 0;
  if (nt_out) *nt_out = 0;
  if ((!text && bytes > 0) || vcap < 0 || tcap < 0 || (vcap > 0 && !verts) || (tcap > 0 && !tris)) return RT_E_INVAL;
  long long nv = 0, nt = 0;
  int line_no = 0;
  std::string num;
  std::vector<long long> face;
  const char* p = text;
  const char* const end = text + bytes;
  while (p < end) {
    ++line_no;
    const char* eol = (const char*)std::memchr(p, '\n', (size_t)(end - p));
    const char* next = eol ? eol + 1 : end;
    const char* le = eol ? eol : end;
    if (const char* hash = (const char*)std::memchr(p, '#', (size_t)(le - p))) le = hash;  // a comment ends the line
    while (p < le && is_space(*p)) ++p;
    while (le > p && is_space(le[-1])) --le;
    const char* kw = p;
    while (p < le && !is_space(*p)) ++p;
    const size_t kwlen = (size_t)(p - kw);
    const bool is_v = kwlen == 1 && *kw == 'v', is_f = kwlen == 1 && *kw == 'f';
    auto fail = [&]() {
      if (err_line) *err_line = line_no;
      return RT_E_INVAL;
    };
    if (is_v) {
      float xyz[3] = {0.0f, 0.0f, 0.0f};
      int count = 0;
      while (true) {
        while (p < le && is_space(*p)) ++p;
        if (p == le) break;
        const char* tok = p;
        while (p < le && !is_space(*p)) ++p;
        num.assign(tok, (size_t)(p - tok));
        char* stop = nullptr;
        const float x = std::strtof(num.c_str(), &stop);
        if (stop == num.c_str() || *stop != '\0') return fail();
        if (count < 3) xyz[count] = x;
        ++count;
      }
      if (count < 3 || nv == INT_MAX) return fail();  // (a fourth number is w, further ones colours: ignored)
      if (nv < vcap) verts[3 * nv] = xyz[0], verts[3 * nv + 1] = xyz[1], verts[3 * nv + 2] = xyz[2];
      ++nv;
    } else if (is_f) {
      face.clear();
      while (true) {
        while (p < le && is_space(*p)) ++p;
        if (p == le) break;
        const char* tok = p;
        while (p < le && !is_space(*p)) ++p;
        long long i;
        if (!parse_face_vertex(tok, p, i)) return fail();
        if (i == 0 || i > nv || i < -nv) return fail();
        face.push_back(i > 0 ? i - 1 : nv + i);
      }
      if (face.size() < 3) return fail();
      for (size_t k = 1; k + 1 < face.size(); ++k) {
        if (nt == RT_MESH_MAX_TRIANGLES) return fail();
        if (nt < tcap) tris[3 * nt] = (int32_t)face[0], tris[3 * nt + 1] = (int32_t)face[k], tris[3 * nt + 2] = (int32_t)face[k + 1];
        ++nt;
      }
    }
    p = next;
  }
  if (nv_out) *nv_out = (int)nv;
  if (nt_out) *nt_out = (int)nt;
  return RT_OK;
}
