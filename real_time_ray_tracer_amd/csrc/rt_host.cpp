// rt_host.cpp — host-only scene/header helpers of the C ABI (no GPU calls).
//
//   rt_pack_sphere/plane/rectangle  <- Application::loadShapeBuffer, src/main.cpp:395-469
//   rt_camera_basis                 <- render(), src/main.cpp:772-779
//   rt_set_mode                     <- compute_one_shader header fill, src/main.cpp:584-585
//   rt_fill_rand_buffer             <- fill_rand_buffer, src/main.cpp:535-539 (seeded)
//   rt_moving_light                 <- moving_light, src/main.cpp:541-551
//   rt_init_scene                   <- init_scene1/5/6, src/scene.h:15-167
//   rt_scenegen                     <- synthetic scenes of SURVEY.md §8d
//   rt_quantize_rgba8               <- the blit into the 8-bit framebuffer, src/main.cpp:783-797
//   rt_resample_rgba8               <- the same blit into a window of another size (GL_LINEAR, 381-388)
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rt/abi.h"

namespace {

struct V3 {
  float x, y, z;
};

V3 cross(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
// glm::normalize: v * inversesqrt(dot(v, v))
V3 normalize(V3 v) {
  float d = v.x * v.x + v.y * v.y + v.z * v.z;
  float inv = 1.0f / std::sqrt(d);
  return V3{v.x * inv, v.y * inv, v.z * inv};
}

float* shape_ptr(float* header, int i) { return header + rt_off_shapes() / 4 + (size_t)i * 20; }

void set4(float* p, float x, float y, float z, float w) {
  p[0] = x;
  p[1] = y;
  p[2] = z;
  p[3] = w;
}

struct SplitMix64 {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  // top 24 bits as a float in [0, 1)
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
  float uniform(float a, float b) { return a + (b - a) * unit(); }
};

const V3 kCamLocation{0.0f, 0.0f, 14.0f};  // src/main.cpp:98
const V3 kCamUp{0.0f, 1.0f, 0.0f};         // src/main.cpp:99
const V3 kCamLook{0.0f, 0.0f, 1.0f};       // src/main.cpp:100

void default_header(float* header, int S, int AA, float aspect, int n_objects) {
  std::memset(header, 0, rt_header_bytes(S, AA));
  rt_set_mode(header, 0, n_objects);
  const float loc[3] = {kCamLocation.x, kCamLocation.y, kCamLocation.z};
  const float up[3] = {kCamUp.x, kCamUp.y, kCamUp.z};
  const float look[3] = {kCamLook.x, kCamLook.y, kCamLook.z};
  rt_camera_basis(header, loc, up, look, aspect);
  set4(header + 4 * RT_HDR_LIGHT_POS, -12.0f, 8.0f, 7.0f, 0.0f);  // DEFAULT_LIGHT_POS, main.cpp:47
  // SKY = vec4(13/255.0, 153/255.0, 219/255.0, 0), main.cpp:44
  set4(header + 4 * RT_HDR_BACKGROUND, (float)(13 / 255.0), (float)(153 / 255.0), (float)(219 / 255.0), 0.0f);
}

}  // namespace

extern "C" {

int rt_pack_sphere(float* header, int S, int i, const float c[3], float r, const float color[3],
                   float reflectivity, int emissive) {
  if (!header || !c || !color || i < 0 || i >= S) return RT_E_INVAL;
  float* s = shape_ptr(header, i);
  set4(s + 0, c[0], c[1], c[2], r);                                  // [0] = (center, radius)
  s[4 + 3] = emissive ? 1.0f : 0.0f;                                 // [1].w = emissive
  s[12 + 3] = reflectivity;                                          // [3].w = reflectivity
  set4(s + 16, color[0], color[1], color[2], (float)RT_SHAPE_SPHERE);  // [4] = (color, id)
  return RT_OK;
}

int rt_pack_plane(float* header, int S, int i, const float n[3], float dist, const float color[3],
                  float reflectivity, int emissive) {
  if (!header || !n || !color || i < 0 || i >= S) return RT_E_INVAL;
  float* s = shape_ptr(header, i);
  V3 nn = normalize(V3{n[0], n[1], n[2]});  // member normal = normalize(normal), plane.h:32
  set4(s + 0, nn.x, nn.y, nn.z, dist);
  s[4 + 3] = emissive ? 1.0f : 0.0f;
  // p0 = dist_from_orig * normal, where `normal` is the constructor PARAMETER (plane.h:33)
  set4(s + 12, dist * n[0], dist * n[1], dist * n[2], reflectivity);
  set4(s + 16, color[0], color[1], color[2], (float)RT_SHAPE_PLANE);
  return RT_OK;
}

int rt_pack_rectangle(float* header, int S, int i, const float llc[3], const float right[3],
                      const float up[3], const float color[3], float reflectivity, int emissive) {
  if (!header || !llc || !right || !up || !color || i < 0 || i >= S) return RT_E_INVAL;
  float* s = shape_ptr(header, i);
  V3 n = normalize(cross(V3{right[0], right[1], right[2]}, V3{up[0], up[1], up[2]}));  // rectangle.h:64
  set4(s + 0, n.x, n.y, n.z, 0.0f);
  set4(s + 4, up[0], up[1], up[2], emissive ? 1.0f : 0.0f);
  set4(s + 8, right[0], right[1], right[2], 0.0f);
  set4(s + 12, llc[0], llc[1], llc[2], reflectivity);
  set4(s + 16, color[0], color[1], color[2], (float)RT_SHAPE_RECTANGLE);
  return RT_OK;
}

int rt_camera_basis(float* header, const float location[3], const float up[3], const float look[3],
                    float aspect) {
  if (!header || !location || !up || !look) return RT_E_INVAL;
  V3 w{look[0], look[1], look[2]};
  V3 u = normalize(cross(V3{up[0], up[1], up[2]}, w));
  V3 v = normalize(cross(w, u));
  V3 h{aspect * u.x, aspect * u.y, aspect * u.z};
  // VERT_ASPECT_RATIO (1.0) * v and -0.5 * (...) use main.cpp's operator*(double, vec3)
  V3 vert{(float)(v.x * 1.0), (float)(v.y * 1.0), (float)(v.z * 1.0)};
  V3 hv{h.x + vert.x, h.y + vert.y, h.z + vert.z};
  V3 llc{(float)(hv.x * -0.5) - w.x, (float)(hv.y * -0.5) - w.y, (float)(hv.z * -0.5) - w.z};
  set4(header + 4 * RT_HDR_HORIZONTAL, h.x, h.y, h.z, 0.0f);
  set4(header + 4 * RT_HDR_VERTICAL, vert.x, vert.y, vert.z, 0.0f);
  set4(header + 4 * RT_HDR_LLC_MINUS_CAMPOS, llc.x, llc.y, llc.z, 0.0f);
  set4(header + 4 * RT_HDR_CAMERA_LOCATION, location[0], location[1], location[2], 0.0f);
  return RT_OK;
}

int rt_set_mode(float* header, int frame, int num_objects) {
  if (!header || frame < 0 || num_objects < 0) return RT_E_INVAL;
  header[4 * RT_HDR_MODE + 1] = (float)frame;
  header[4 * RT_HDR_MODE + 2] = (float)num_objects;
  return RT_OK;
}

int rt_fill_rand_buffer(float* header, int S, int AA, uint64_t seed) {
  if (!header || S < 0 || AA <= 0) return RT_E_INVAL;
  SplitMix64 g{seed};
  float* rb = header + rt_off_rand(S) / 4;
  for (int i = 0; i < AA * 2 * 4; ++i) rb[i] = g.unit();
  return RT_OK;
}

int rt_moving_light(float* header, int light_movement) {
  if (!header) return RT_E_INVAL;
  float* L = header + 4 * RT_HDR_LIGHT_POS;
  if (light_movement) {
    for (int k = 0; k < 4; ++k) L[k] = L[k] + 0.1f;  // light_pos + vec4(0.1)
    if (L[0] > 50.0f) set4(L, -50.0f, 20.0f, -50.0f, 0.0f);
  } else {
    set4(L, -12.0f, 8.0f, 7.0f, 0.0f);
  }
  return RT_OK;
}

int rt_scenegen(float* header, int S, int n_objects, int AA, uint64_t seed, float aspect) {
  if (!header || S < 0 || n_objects < 0 || n_objects > S || AA <= 0) return RT_E_INVAL;
  default_header(header, S, AA, aspect, n_objects);
  SplitMix64 g{seed};
  for (int i = 0; i < n_objects; ++i) {
    if (i == 0) {  // ground, as scene5/6 (src/scene.h:96-99)
      const float c[3] = {0.0f, -35.0f, 0.0f}, col[3] = {0.8f, 0.6f, 0.2f};
      rt_pack_sphere(header, S, 0, c, 33.0f, col, 1.0f, 0);
      continue;
    }
    float c[3] = {g.uniform(-12.0f, 12.0f), g.uniform(-2.0f, 6.0f), g.uniform(-20.0f, 4.0f)};
    float r = g.uniform(0.3f, 1.5f);
    float col[3] = {g.uniform(0.1f, 0.9f), g.uniform(0.1f, 0.9f), g.uniform(0.1f, 0.9f)};
    float p_refl = g.unit(), refl_v = g.uniform(0.0f, 0.6f), p_emis = g.unit();
    float refl = p_refl < 0.6f ? 1.0f : refl_v;
    int emissive = p_emis < (1.0f / 16.0f);
    if (emissive)
      for (float& k : col) k *= 4.0f;
    rt_pack_sphere(header, S, i, c, r, col, refl, emissive);
  }
  return rt_fill_rand_buffer(header, S, AA, 7000);
}

int rt_init_scene(float* header, int S, int AA, int which, float aspect) {
  if (!header || AA <= 0) return RT_E_INVAL;
  struct Sph {
    float c[3], r, col[3], refl;
    int emis;
  };
  if (which == 1) {  // src/scene.h:15-65
    if (S < 5) return RT_E_INVAL;
    default_header(header, S, AA, aspect, 5);
    const Sph sp[4] = {{{0, -0.5f, 0}, 2, {0.8f, 0.2f, 0.5f}, 0.5f, 0},
                       {{4, -0.5f, -2}, 3.5f, {0.8f, 0.8f, 0.1f}, 0.9f, 0},
                       {{-4.5f, 4, -15}, 4, {0.2f, 0.8f, 0.1f}, 0.2f, 0},
                       {{-8, -1, 2}, 1.5f, {1, 1, 1}, 0.0f, 0}};
    for (int i = 0; i < 4; ++i) rt_pack_sphere(header, S, i, sp[i].c, sp[i].r, sp[i].col, sp[i].refl, sp[i].emis);
    const float n[3] = {0, 1, 0}, col[3] = {0.3f, 0.0f, 0.5f};
    rt_pack_plane(header, S, 4, n, -4.0f, col, 1.0f, 0);
  } else if (which == 5) {  // src/scene.h:67-109
    if (S < 3) return RT_E_INVAL;
    default_header(header, S, AA, aspect, 3);
    const Sph sp[3] = {{{0, 18, 0}, 10, {1.5f, 1.5f, 1.5f}, 1.0f, 1},
                       {{0, 0, 0}, 2, {0.2f, 0.6f, 0.8f}, 0.4f, 0},
                       {{0, -35, 0}, 33, {0.8f, 0.6f, 0.2f}, 1.0f, 0}};
    for (int i = 0; i < 3; ++i) rt_pack_sphere(header, S, i, sp[i].c, sp[i].r, sp[i].col, sp[i].refl, sp[i].emis);
  } else if (which == 7) {  // scene 5 with the rectangle area light the reference left commented out (src/scene.h:80-86)
    if (S < 3) return RT_E_INVAL;
    default_header(header, S, AA, aspect, 3);
    const float llc[3] = {4, 6, 4}, right[3] = {0, 0, -8}, up[3] = {-8, 0, 0}, col[3] = {1.5f, 1.5f, 1.5f};
    rt_pack_rectangle(header, S, 0, llc, right, up, col, 1.0f, 1);
    const Sph sp[2] = {{{0, 0, 0}, 2, {0.2f, 0.6f, 0.8f}, 0.4f, 0}, {{0, -35, 0}, 33, {0.8f, 0.6f, 0.2f}, 1.0f, 0}};
    for (int i = 0; i < 2; ++i) rt_pack_sphere(header, S, 1 + i, sp[i].c, sp[i].r, sp[i].col, sp[i].refl, sp[i].emis);
  } else if (which == 6) {  // src/scene.h:111-167
    if (S < 6) return RT_E_INVAL;
    default_header(header, S, AA, aspect, 6);
    const Sph sp[6] = {{{0, 12, 0}, 6, {4, 4, 4}, 1.0f, 1},
                       {{-8, 0, 0}, 2, {8, 8, 16}, 1.0f, 1},
                       {{0, 0, 0}, 2, {0.2f, 0.6f, 0.8f}, 0.4f, 0},
                       {{0, -35, 0}, 33, {0.8f, 0.6f, 0.2f}, 1.0f, 0},
                       {{2, 1, 3}, 0.5f, {1, 1, 1}, 0.0f, 0},
                       {{4.5f, 0.2f, 5}, 2.25f, {1, 1, 1}, 0.0f, 0}};
    for (int i = 0; i < 6; ++i) rt_pack_sphere(header, S, i, sp[i].c, sp[i].r, sp[i].col, sp[i].refl, sp[i].emis);
  } else {
    return RT_E_INVAL;
  }
  return rt_fill_rand_buffer(header, S, AA, 7000);
}

// The blit's 8-bit conversion (src/main.cpp:783-797, shader_fragment.glsl:9-19), the rule
// present_kernel (rt_kernels_impl.h) implements on the device: NaN and v <= 0 give 0, v >= 1 gives
// 255, else v * 255 + 0.5 in binary32 (no contraction: this file is built with -ffp-contract=off)
// truncated; alpha is 255.
int rt_quantize_rgba8(const float* image, int width, int rows, int top_down, uint8_t* out) {
  if (!image || !out || width <= 0 || rows <= 0) return RT_E_INVAL;
  for (int j = 0; j < rows; ++j) {
    const float* src = image + (size_t)(top_down ? rows - 1 - j : j) * width * 4;
    uint8_t* dst = out + (size_t)j * width * 4;
    for (int x = 0; x < width; ++x) {
      for (int c = 0; c < 3; ++c) {
        const float v = src[4 * x + c];
        uint8_t q = 0;  // NaN fails both comparisons below
        if (v >= 1.0f) q = 255;
        else if (v > 0.0f) q = (uint8_t)(int)(v * 255.0f + 0.5f);
        dst[4 * x + c] = q;
      }
      dst[4 * x + 3] = 255;
    }
  }
  return RT_OK;
}

}  // extern "C"

namespace {

// One axis of the blit's GL_LINEAR sampling (src/main.cpp:381-388, 783-797): output sample i of
// `dst` over `src` texels sits at texel coordinate (2i + 1) * src / (2 * dst) - 1/2 = n / d - 1 in
// integers; i0 is its floor, w the fraction (one correctly rounded binary32 division of two exact
// operands, rem < d <= 2^15).  GL_CLAMP_TO_EDGE moves the tap indices only, never the weight.
struct ScaleTap {
  int i0, i1;
  float w;
};
ScaleTap scale_tap(int i, int src, int dst) {
  const int n = (2 * i + 1) * src - dst, d = 2 * dst;      // n + d > 0; all below 2^30
  const int x0 = (int)((unsigned)(n + d) / (unsigned)d) - 1;  // floor(n / d)
  const int rem = n - x0 * d;                              // 0 <= rem < d
  const int hi = src - 1;
  return ScaleTap{x0 < 0 ? 0 : (x0 > hi ? hi : x0), x0 + 1 < 0 ? 0 : (x0 + 1 > hi ? hi : x0 + 1),
                  (float)rem / (float)d};
}
// the select on a zero weight is part of the rule: that tap's texel (NaN, inf) does not reach the result
inline float scale_mix(float w, float t0, float t1) { return w == 0.0f ? t0 : ((1.0f - w) * t0 + w * t1); }

inline uint8_t quantize_channel(float v) {  // rt_quantize_rgba8's rule
  if (v >= 1.0f) return 255;
  if (v > 0.0f) return (uint8_t)(int)(v * 255.0f + 0.5f);
  return 0;  // NaN fails both comparisons
}

}  // namespace

extern "C" {

// The blit at window size (src/main.cpp:783-797 with the texture's GL_LINEAR / GL_CLAMP_TO_EDGE,
// 381-388), the rule present_scaled_kernel (rt_kernels_impl.h) implements on the device: per output
// pixel the two taps and the weight of each axis (scale_tap), per channel the blend along x on both
// source rows, then along y, in binary32 without contraction, then rt_quantize_rgba8's conversion.
int rt_resample_rgba8(const float* image, int width, int rows, int out_width, int out_rows, int top_down,
                      uint8_t* out) {
  const int lim = RT_PRESENT_SCALED_MAX;
  if (!image || !out || width < 1 || rows < 1 || out_width < 1 || out_rows < 1 || width > lim || rows > lim ||
      out_width > lim || out_rows > lim)
    return RT_E_INVAL;
  std::vector<ScaleTap> tx((size_t)out_width);
  for (int i = 0; i < out_width; ++i) tx[i] = scale_tap(i, width, out_width);
  for (int j = 0; j < out_rows; ++j) {
    const ScaleTap ty = scale_tap(top_down ? out_rows - 1 - j : j, rows, out_rows);
    const float* r0 = image + (size_t)ty.i0 * width * 4;
    const float* r1 = image + (size_t)ty.i1 * width * 4;
    uint8_t* dst = out + (size_t)j * out_width * 4;
    for (int i = 0; i < out_width; ++i) {
      const size_t a0 = (size_t)tx[i].i0 * 4, a1 = (size_t)tx[i].i1 * 4;
      for (int c = 0; c < 3; ++c) {
        const float h0 = scale_mix(tx[i].w, r0[a0 + c], r0[a1 + c]);
        const float h1 = scale_mix(tx[i].w, r1[a0 + c], r1[a1 + c]);
        dst[4 * i + c] = quantize_channel(scale_mix(ty.w, h0, h1));
      }
      dst[4 * i + 3] = 255;
    }
  }
  return RT_OK;
}

}  // extern "C"
