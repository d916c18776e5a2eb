// rt_query_host.cpp — the ray queries' rules in plain C++ on a header (include/rt/abi.h "Ray
// queries"): the specification of rt_trace_rays / rt_trace_pixels / rt_occluded.  Host only, no HIP
// header; built with -ffp-contract=off like rt_host.cpp, every fused operation written as fmaf, so
// the float semantics are the ones oracle/rt_oracle.h states.
//
//   eval_ray, sphere_eval_ray, plane_eval_ray   p_compute.glsl:77-138
//   the rectangle rule (flags RT_SCENE_RECTANGLES) include/rt/abi.h "Rectangles"
//   the closest-hit loop                        p_compute.glsl:177-188 (h_ 199-210, ao_ 183-194)
//   the primary ray                             p_compute.glsl:233-235
//   shadow_ray                                  p_compute.glsl:145-166
#include <cmath>
#include <cstdint>

#include "../../include/rt/abi.h"

namespace {

struct V3 {
  float x, y, z;
};

V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 scale(float s, V3 v) { return V3{s * v.x, s * v.y, s * v.z}; }
V3 at(const float* p, size_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
// GLSL dot(): a fused chain
float dot(V3 a, V3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
// GLSL normalize(): v * (1 / sqrt(dot(v, v))), IEEE square root and division
V3 normalize(V3 v) {
  const float il = 1.0f / std::sqrt(dot(v, v));
  return V3{v.x * il, v.y * il, v.z * il};
}

float sphere_eval(V3 pos, V3 dir, const float* g) {
  const V3 pmc = sub(pos, V3{g[0], g[1], g[2]});
  const float b = dot(dir, pmc);
  const float del = std::fmaf(g[3], g[3], std::fmaf(b, b, -dot(pmc, pmc)));
  if (del < 0.0f) return -1.0f;
  if (del == 0.0f) return -1.0f * b;
  const float s = std::sqrt(del);
  const float t1 = -1.0f * b + s;
  const float t2 = -1.0f * b - s;
  if (t2 < 0.0f) return t1 < 0.0f ? -1.0f : t1;
  return t2;
}

float plane_eval(V3 pos, V3 dir, const float* n4, const float* p04) {
  const V3 n{n4[0], n4[1], n4[2]};
  const float denom = dot(n, dir);
  if (denom < 0.001f && denom > -0.001f) return -1.0f;
  return dot(n, sub(V3{p04[0], p04[1], p04[2]}, pos)) / denom;
}

// The rectangle rule (include/rt/abi.h "Rectangles") on row sh as loadShapeBuffer packs it
// (src/main.cpp:444-467): n = [0].xyz, up = [1].xyz, right = [2].xyz, llc = [3].xyz.  plane_eval_ray
// with p0 = llc, then the hit point's two slabs; edges inclusive, a NaN fails a comparison.
float rectangle_eval(V3 pos, V3 dir, const float* sh) {
  const V3 n{sh[0], sh[1], sh[2]}, up{sh[4], sh[5], sh[6]}, right{sh[8], sh[9], sh[10]}, llc{sh[12], sh[13], sh[14]};
  const float den = dot(n, dir);
  if (den < 0.001f && den > -0.001f) return -1.0f;
  const float t = dot(n, sub(llc, pos)) / den;
  const V3 q = sub(add(pos, scale(t, dir)), llc);  // one multiply, one add, one subtract per component
  const float a = dot(q, right), b = dot(q, up);
  return (a >= 0.0f && a <= dot(right, right) && b >= 0.0f && b <= dot(up, up)) ? t : -1.0f;
}

// a header checked against its configuration
struct Scene {
  const float* hdr;
  const float* shapes;  // simple_shapes[S][5] vec4
  int nobj;
  bool rects;  // RT_SCENE_RECTANGLES: shape id 3 follows rectangle_eval (else it is never hit)
};

// int(simple_shapes[i][4].w), 0 for a value no int holds (as the device table's packing)
int shape_id(const Scene& s, int i) {
  const float idf = s.shapes[(size_t)i * 20 + 16 + 3];
  return (idf > -2147483648.0f && idf < 2147483648.0f) ? (int)idf : 0;
}

float eval_ray(const Scene& s, V3 pos, V3 dir, int i) {
  const float* sh = s.shapes + (size_t)i * 20;
  const int id = shape_id(s, i);
  if (id == RT_SHAPE_SPHERE) return sphere_eval(pos, dir, sh);
  if (id == RT_SHAPE_PLANE) return plane_eval(pos, dir, sh, sh + 12);
  if (id == RT_SHAPE_RECTANGLE && s.rects) return rectangle_eval(pos, dir, sh);
  return -1.0f;
}

int open_scene(const rt_config* cfg, const void* header, size_t header_bytes, int flags, Scene& s) {
  if ((flags & ~RT_SCENE_RECTANGLES) != 0) return RT_E_INVAL;
  s.rects = (flags & RT_SCENE_RECTANGLES) != 0;
  if (!cfg || !header || cfg->num_shapes < 0 || cfg->spp <= 0 ||
      header_bytes != rt_header_bytes(cfg->num_shapes, cfg->spp))
    return RT_E_INVAL;
  s.hdr = (const float*)header;
  s.shapes = s.hdr + rt_off_shapes() / 4;
  const float mz = s.hdr[RT_HDR_MODE * 4 + 2];  // int(mode.z) must lie in [0, S]
  if (!(mz >= 0.0f && mz < (float)(cfg->num_shapes + 1))) return RT_E_INVAL;
  s.nobj = (int)mz;
  return RT_OK;
}

bool thr_ok(float thr) { return thr >= 0.0f && thr <= 3.402823466e+38f; }  // finite and >= 0; NaN fails

}  // namespace

extern "C" {

float rt_rectangle_eval_host(const float shape[20], const float pos[3], const float dir[3]) {
  if (!shape || !pos || !dir) return -1.0f;
  return rectangle_eval(V3{pos[0], pos[1], pos[2]}, V3{dir[0], dir[1], dir[2]}, shape);
}

int rt_trace_rays_host(const rt_config* cfg, const void* header, size_t header_bytes, const float* origins,
                       const float* dirs, size_t n, float thr, float* t_out, int32_t* ind_out, float* normals) {
  return rt_trace_rays_host_ex(cfg, header, header_bytes, origins, dirs, n, thr, 0, t_out, ind_out, normals);
}

int rt_trace_rays_host_ex(const rt_config* cfg, const void* header, size_t header_bytes, const float* origins,
                          const float* dirs, size_t n, float thr, int flags, float* t_out, int32_t* ind_out,
                          float* normals) {
  Scene s;
  int rc = open_scene(cfg, header, header_bytes, flags, s);
  if (rc != RT_OK) return rc;
  if (n > RT_QUERY_MAX_RAYS || !thr_ok(thr)) return RT_E_INVAL;
  if (n == 0) return RT_OK;
  if (!origins || !dirs) return RT_E_INVAL;
  for (size_t k = 0; k < n; ++k) {
    const V3 o = at(origins, k), d = at(dirs, k);
    float t = -1.0f;
    int ind = -1;
    for (int i = 0; i < s.nobj; ++i) {
      const float res = eval_ray(s, o, d, i);
      if (res > thr && (res < t || t < 0.0f)) {
        t = res;
        ind = i;
      }
    }
    if (t_out) t_out[k] = t;
    if (ind_out) ind_out[k] = ind;
    if (normals) {
      V3 nn{0.0f, 0.0f, 0.0f};
      if (ind >= 0) {
        const float* g = s.shapes + (size_t)ind * 20;
        // the hit point: one multiply and one add per component
        if (shape_id(s, ind) == RT_SHAPE_SPHERE) nn = normalize(sub(add(o, scale(t, d)), V3{g[0], g[1], g[2]}));
        else nn = V3{g[0], g[1], g[2]};
      }
      normals[3 * k] = nn.x;
      normals[3 * k + 1] = nn.y;
      normals[3 * k + 2] = nn.z;
    }
  }
  return RT_OK;
}

int rt_pixel_rays_host(const rt_config* cfg, const void* header, size_t header_bytes, const int32_t* xy, size_t n,
                       float* origins, float* dirs) {
  Scene s;
  int rc = open_scene(cfg, header, header_bytes, 0, s);
  if (rc != RT_OK) return rc;
  if (cfg->width <= 0 || cfg->height <= 0 || n > RT_QUERY_MAX_RAYS) return RT_E_INVAL;
  if (n == 0) return RT_OK;
  if (!xy) return RT_E_INVAL;
  const float* h = s.hdr;
  const V3 hor{h[4 * RT_HDR_HORIZONTAL], h[4 * RT_HDR_HORIZONTAL + 1], h[4 * RT_HDR_HORIZONTAL + 2]};
  const V3 ver{h[4 * RT_HDR_VERTICAL], h[4 * RT_HDR_VERTICAL + 1], h[4 * RT_HDR_VERTICAL + 2]};
  const V3 llc{h[4 * RT_HDR_LLC_MINUS_CAMPOS], h[4 * RT_HDR_LLC_MINUS_CAMPOS + 1], h[4 * RT_HDR_LLC_MINUS_CAMPOS + 2]};
  const float* cam = h + 4 * RT_HDR_CAMERA_LOCATION;
  const float fW = (float)cfg->width, fH = (float)cfg->height;
  for (size_t k = 0; k < n; ++k) {
    const float hp = (float)xy[2 * k] / fW, vp = (float)xy[2 * k + 1] / fH;
    const V3 d = normalize(add(add(llc, scale(hp, hor)), scale(vp, ver)));
    if (origins) {
      origins[3 * k] = cam[0];
      origins[3 * k + 1] = cam[1];
      origins[3 * k + 2] = cam[2];
    }
    if (dirs) {
      dirs[3 * k] = d.x;
      dirs[3 * k + 1] = d.y;
      dirs[3 * k + 2] = d.z;
    }
  }
  return RT_OK;
}

int rt_occluded_host(const rt_config* cfg, const void* header, size_t header_bytes, const float* from,
                     const float* to, size_t n, uint8_t* out) {
  return rt_occluded_host_ex(cfg, header, header_bytes, from, to, n, 0, out);
}

int rt_occluded_host_ex(const rt_config* cfg, const void* header, size_t header_bytes, const float* from,
                        const float* to, size_t n, int flags, uint8_t* out) {
  Scene s;
  int rc = open_scene(cfg, header, header_bytes, flags, s);
  if (rc != RT_OK) return rc;
  if (n > RT_QUERY_MAX_RAYS) return RT_E_INVAL;
  if (n == 0) return RT_OK;
  if (!from || !to) return RT_E_INVAL;
  if (!out) return RT_OK;
  for (size_t k = 0; k < n; ++k) {
    const V3 pos = at(from, k), lv = sub(at(to, k), pos);
    const V3 l = normalize(lv);
    const float len = std::sqrt(dot(lv, lv));
    const V3 np = add(pos, scale(0.01f, l));
    uint8_t occ = 0;
    for (int i = 0; i < s.nobj && !occ; ++i) {
      const double t = (double)eval_ray(s, np, l, i);
      if (t > (double)0.0001f) {  // the shader's double t against its float literal
        const double dx = t * (double)l.x, dy = t * (double)l.y, dz = t * (double)l.z;
        if (std::sqrt(std::fma(dz, dz, std::fma(dy, dy, dx * dx))) < (double)len) occ = 1;
      }
    }
    out[k] = occ;
  }
  return RT_OK;
}

}  // extern "C"
