// rt_mesh_rule.h — the mesh rule's arithmetic (include/rt/mesh.h "The rule"), written once for the
// host specification (rt_mesh_host.cpp, plain C++) and the kernels (rt_mesh_kernels.hip): the same
// operations on the same operands in the same order.  Both sides are compiled with
// -ffp-contract=off; every fused operation is written as fmaf; '/' and sqrt are the IEEE ones.
#pragma once
#include <float.h>
#include <stdint.h>

// (the kernels' unit defines RT_MESH_RULE_DEVICE before it includes this file)
#ifdef RT_MESH_RULE_DEVICE
#define RT_MESH_HD __host__ __device__ __forceinline__
#else
#define RT_MESH_HD inline
#endif

namespace rt {
namespace mesh {

struct V3 {
  float x, y, z;
};

RT_MESH_HD V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_MESH_HD float dot(V3 a, V3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
// two products and one subtraction per component
RT_MESH_HD V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RT_MESH_HD float mn(float a, float b) { return a < b ? a : b; }
RT_MESH_HD float mx(float a, float b) { return a > b ? a : b; }
RT_MESH_HD V3 mn(V3 a, V3 b) { return V3{mn(a.x, b.x), mn(a.y, b.y), mn(a.z, b.z)}; }
RT_MESH_HD V3 mx(V3 a, V3 b) { return V3{mx(a.x, b.x), mx(a.y, b.y), mx(a.z, b.z)}; }
RT_MESH_HD bool finite(float x) { return __builtin_fabsf(x) <= FLT_MAX; }  // false for NaN
RT_MESH_HD bool finite(V3 v) { return finite(v.x) && finite(v.y) && finite(v.z); }
// GLSL normalize(): v * (1 / sqrt(dot(v, v)))
RT_MESH_HD V3 normalize(V3 v) {
  const float il = 1.0f / __builtin_sqrtf(dot(v, v));
  return V3{v.x * il, v.y * il, v.z * il};
}

// A ray with what box_pass needs of it once: 1.0f / d_a of the axes that contribute an interval
// (the value box_pass's rule computes per test), and the mask of the zero (or subnormal) axes.
struct Ray {
  V3 o, d, inv;
  int zero;  // bit a: |d_a| < FLT_MIN
  bool ok;   // the ray gate: every component of o and d finite
};

RT_MESH_HD Ray make_ray(V3 o, V3 d) {
  Ray r;
  r.o = o;
  r.d = d;
  r.ok = finite(o) && finite(d);
  r.zero = (__builtin_fabsf(d.x) < FLT_MIN ? 1 : 0) | (__builtin_fabsf(d.y) < FLT_MIN ? 2 : 0) |
           (__builtin_fabsf(d.z) < FLT_MIN ? 4 : 0);
  r.inv = V3{(r.zero & 1) ? 0.0f : 1.0f / d.x, (r.zero & 2) ? 0.0f : 1.0f / d.y, (r.zero & 4) ? 0.0f : 1.0f / d.z};
  return r;
}

// one axis of box_pass: false if a zero axis fails its interval test
RT_MESH_HD bool box_axis(bool zero, float o, float inv, float lo, float hi, float& tn, float& tf) {
  if (zero) return lo <= o && o <= hi;
  const float t1 = (lo - o) * inv, t2 = (hi - o) * inv;
  tn = mx(tn, mn(t1, t2));
  tf = mn(tf, mx(t1, t2));
  return true;
}

RT_MESH_HD bool box_pass(const Ray& r, V3 lo, V3 hi) {
  float tn = -__builtin_inff(), tf = __builtin_inff();
  const bool zx = box_axis(r.zero & 1, r.o.x, r.inv.x, lo.x, hi.x, tn, tf);
  const bool zy = box_axis(r.zero & 2, r.o.y, r.inv.y, lo.y, hi.y, tn, tf);
  const bool zz = box_axis(r.zero & 4, r.o.z, r.inv.z, lo.z, hi.z, tn, tf);
  return zx && zy && zz && tf >= 0.0f && tn <= tf * 1.000003814697265625f;
}

struct Hit {
  float t, u, v;
};

RT_MESH_HD Hit tri_eval(const Ray& r, V3 v0, V3 v1, V3 v2) {
  const Hit miss{-1.0f, 0.0f, 0.0f};
  if (!box_pass(r, mn(mn(v0, v1), v2), mx(mx(v0, v1), v2))) return miss;
  const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  const V3 p = cross(r.d, e2);
  const float det = dot(e1, p);
  if (!(det != 0.0f)) return miss;
  const float inv = 1.0f / det;
  const V3 s = sub(r.o, v0);
  const float u = dot(s, p) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return miss;
  const V3 q = cross(s, e1);
  const float v = dot(r.d, q) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return miss;
  return Hit{dot(e2, q) * inv, u, v};
}

// The closest-hit loop's acceptance, order-free: the candidate (t, i) against the best so far; what
// the ascending loop `t > thr && (t < best || best < 0)` keeps, whatever the visiting order.
RT_MESH_HD bool closer(float t, int i, float thr, float best_t, int best_i) {
  return t > thr && (best_t < 0.0f || t < best_t || (t == best_t && i < best_i));
}

RT_MESH_HD V3 tri_normal(V3 v0, V3 v1, V3 v2) { return normalize(cross(sub(v1, v0), sub(v2, v0))); }

// The occlusion segment a -> b: the ray (a + 0.01f * l, l) and the segment's length.
RT_MESH_HD Ray segment_ray(V3 a, V3 b, float& len) {
  const V3 lv = sub(b, a);
  const V3 l = normalize(lv);
  len = __builtin_sqrtf(dot(lv, lv));
  const V3 t{0.01f * l.x, 0.01f * l.y, 0.01f * l.z};
  return make_ray(V3{a.x + t.x, a.y + t.y, a.z + t.z}, l);
}

// rt_occluded's binary64 test for one triangle's float t: t > 0.0001f and length(dvec3(t * l)) < len
RT_MESH_HD bool occludes(float tf, V3 l, double dlen) {
  if (!(tf > 0.0001f)) return false;
  const double t = (double)tf;
  const double dx = t * (double)l.x, dy = t * (double)l.y, dz = t * (double)l.z;
  return __builtin_sqrt(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx))) < dlen;
}

// The merge of RT_MESH_MERGE: does the mesh's hit (prim >= 0) replace the existing answer t_old?
RT_MESH_HD bool merge_takes(float t_mesh, int prim, float t_old) { return prim >= 0 && (t_old < 0.0f || t_mesh < t_old); }

}  // namespace mesh
}  // namespace rt
