// rt_kernels_impl.h — the gfx950 kernels of the per-pixel ray-scene hot path (device code and
// kernel templates), included by the production launcher (rt_kernels.hip) and by the A/B tools
// library (tools/ab/rt_kernels_ab.hip, make ablib).
//
//   phong_kernel     <- resources/p_compute.glsl   (mode 3)
//   hybrid_kernel    <- resources/h_compute.glsl   (mode 4)
//   phong_gbuf_kernel, hybrid_gbuf_kernel: the same two, also storing the primary hit's normal and
//                       depth as the AO shaders do (rt_set_phong_gbuffer; the reference has no such shader)
//   ao_batch_kernel  <- resources/ao_compute.glsl  (mode 2) / aop_compute.glsl (mode 1 pass 1)
//   post_kernel      <- resources/aop_postprocessing.glsl (mode 1 pass 2)
//
// The reference dispatches W x H single-lane workgroups (local_size 1x1, p_compute.glsl:26).
// Here a 256-lane workgroup (4 wave64) owns a 16x16 pixel tile (modes 3/4, one lane per
// pixel), and a one-wave workgroup owns a pool of 256 pixel-samples (modes 1/2).  The sphere
// table is read on the scalar path with wave-uniform loads; camera rays are cone-culled per
// wave / pool.  Planes are tested after the spheres of each segment.  Per-sample AO results are
// combined in sample order, so the sum order matches the reference's sequential
// `result_color += ambient_occlusion(dir, aa)` (ao_compute.glsl:303-330).
//
// The kernel templates carry diagnostic parameters (ABL: timing ablations, section clocks and
// event counts; !ALLSPH: the unculled LDS-table Phong/hybrid kernels) that only the A/B tools
// library instantiates; the production launcher (launch_production below) never does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/rt/abi.h"
#include "rt_device.h"
#include "rt_kernels.h"

namespace rt {

namespace {

constexpr int kBlock = 256;
constexpr float kGamma = 1.0f / 2.2f;  // p_compute.glsl:240

// Stage the first nobj entries of the four [S] tables into LDS as [4][nobj].
__device__ __forceinline__ void stage_shapes(const FrameParams& P, float4* lds) {
  const int n = P.nobj;
  for (int k = threadIdx.x; k < 4 * n; k += blockDim.x) {
    int tab = k / n, i = k - tab * n;
    lds[k] = P.shapes[(size_t)tab * P.S + i];
  }
}

// P: anything with the camera's lx.. / hx.. / vx.. members (FrameParams, QueryScene)
template <class Cam>
__device__ __forceinline__ f3 primary_dir(const Cam& P, float hp, float vp) {
  // normalize(llc_minus_campos + hp*horizontal + vp*vertical), p_compute.glsl:235
  f3 a = mk(P.lx + hp * P.hx, P.ly + hp * P.hy, P.lz + hp * P.hz);
  return normalize(mk(a.x + vp * P.vx, a.y + vp * P.vy, a.z + vp * P.vz));
}

__device__ __forceinline__ float4 gamma_out(float r, float g, float b) {
  // pow(c, 1/2.2) as exp2(log2(c) / 2.2) on the hardware v_log_f32 / v_exp_f32: relative
  // error ~5e-6 at worst (|log2 c| <= 126), inside the 1e-4 output tolerance; outputs only,
  // never feeds control flow (0 -> 0, inf -> inf, NaN -> NaN as powf)
  auto gm = [](float c) { return __builtin_amdgcn_exp2f(kGamma * __builtin_amdgcn_logf(c)); };
  return make_float4(gm(r), gm(g), gm(b), 0.0f);
}

// pow(x, 500) of the specular term (p_compute.glsl:230, h_compute.glsl:266) for x = clamp(.., 0,
// 1), by squaring: x^500 = x^256 x^128 x^64 x^32 x^16 x^4, 13 multiplies instead of powf's
// extended-precision log/exp.  Each squaring at most doubles the relative error and adds half an
// ulp, so the result is within ~500 ulp (3e-5 relative) of x^500 while it is normal, and below
// 1e-38 (the tolerance's 1e-6 absolute slack) where intermediate powers go subnormal.  The term
// only feeds the colour (never control flow); 0 -> 0, 1 -> 1, NaN -> NaN as powf.
__device__ __forceinline__ float pow500(float x) {
  const float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8, x32 = x16 * x16, x64 = x32 * x32,
              x128 = x64 * x64, x256 = x128 * x128;
  return ((((x256 * x128) * x64) * x32) * x16) * x4;
}

// 8x8 pixels per wave (ray coherence inside a wave), BWX x BWY waves per block (16x16 pixels
// per 256-lane block by default); block tile (bx, by) of the trace rows.
template <int BWX = 2, int BWY = 2>
__device__ __forceinline__ void tile_xy(int& x, int& y, int row0, int bx, int by) {
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  x = bx * 8 * BWX + (wave % BWX) * 8 + (lane & 7);
  y = row0 + by * 8 * BWY + (wave / BWX) * 8 + (lane >> 3);
}
__device__ __forceinline__ void tile_xy(int& x, int& y, int row0) { tile_xy<2, 2>(x, y, row0, blockIdx.x, blockIdx.y); }

// Work counters for the algorithmic-FLOP roofline (only when P.counters is set).  Called by
// every lane of a wave with the wave converged; one atomic per counter per wave.
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o));
  return v;
}
// Float wave reductions over all 64 lanes on the DPP path (quad perms, row mirrors, row
// broadcasts), result read from lane 63 (wave-uniform).  The whole wave must be active.
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROWMASK, 0xf, false));
}
template <typename Op>
__device__ __forceinline__ float wave_reduce_f(float v, Op op) {
  v = op(v, dpp_f<0xB1>(v));        // quad_perm [1,0,3,2]
  v = op(v, dpp_f<0x4E>(v));        // quad_perm [2,3,0,1]
  v = op(v, dpp_f<0x141>(v));       // row_half_mirror: 8 lanes
  v = op(v, dpp_f<0x140>(v));       // row_mirror: 16 lanes
  v = op(v, dpp_f<0x142, 0xA>(v));  // row_bcast:15 into rows 1, 3
  v = op(v, dpp_f<0x143, 0xC>(v));  // row_bcast:31 into rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_min_f(float v) { return wave_reduce_f(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max_f(float v) { return wave_reduce_f(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ float wave_sum_f(float v) { return wave_reduce_f(v, [](float a, float b) { return a + b; }); }

__device__ __forceinline__ void count_work(const FrameParams& P, bool active, int y, unsigned segs, unsigned shadows) {
  if (P.row_counters && active) atomicAdd(&P.row_counters[y - P.band_row0], (unsigned long long)(segs + shadows));
  if (!P.counters) return;
  if (!active) segs = shadows = 0;
  unsigned n = wave_sum(active ? 1u : 0u), sg = wave_sum(segs), sh = wave_sum(shadows);
  unsigned slots = wave_max(segs + shadows) * 64u;  // lane slots spent in scene loops (divergence)
  if ((threadIdx.x & 63) == 0) {
    // kCounterSlots copies per counter, spread by wave id, so waves do not serialise on one
    // address; the host sums the slots
    unsigned long long* c = P.counters + ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (kCounterSlots - 1));
    atomicAdd(&c[0 * kCounterSlots], (unsigned long long)n);
    atomicAdd(&c[1 * kCounterSlots], (unsigned long long)sg);
    atomicAdd(&c[2 * kCounterSlots], (unsigned long long)sh);
    atomicAdd(&c[3 * kCounterSlots], (unsigned long long)(sg + sh) * (unsigned long long)P.nobj);
    atomicAdd(&c[4 * kCounterSlots], (unsigned long long)slots * (unsigned long long)P.nobj);
  }
}

// Colour stores (g-buffer slot + image) non-temporal: written once, read by a later launch at
// the earliest.  Hybrid (b) 26.25 -> 25.78 us, post_kernel (d) 0.311 -> 0.293 ms, AO and Phong
// unchanged (profiles/r05u_*).  The AO pass's normal and depth stores stay plain stores.
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt(float4* p, float4 c) {
  __builtin_nontemporal_store(f4v{c.x, c.y, c.z, c.w}, (f4v*)p);
}
__device__ __forceinline__ void store_color(const FrameParams& P, float4* out_pix, float4* image, int x, int y,
                                            float4 c) {
  float4* const po = out_pix + (size_t)(y - P.band_row0) * P.W + x;
  st_nt(po, c);
  if (image) {
    int r = y - P.img_row0;
    if (r >= 0 && r < P.img_rows) {
      st_nt(image + (size_t)r * P.W + x, c);
    }
  }
}
__device__ __forceinline__ void store_color(const FrameParams& P, int x, int y, float4 c) {
  store_color(P, P.out_pix, P.image, x, y, c);
}

// The frame a Phong/hybrid block renders: its light, colour slot and image (multi-frame
// launches: frame blockIdx.z of the batch, see FrameParams::mf_n).
// Depth g-buffer slot layout: two planes of [band_rows][W] float2, (x, y) then (z, w).  The
// post-process reads only depth.x and depth.y (aop_postprocessing.glsl: the neighbour weights and
// the history test), so it reads 8 B per depth instead of 16; the AO pass writes both planes and
// reads both for its stale-depth pixels.  rt_download / rt_upload_gbuffer convert to the
// reference's vec4 layout.
__device__ __forceinline__ size_t dep_plane(const FrameParams& P) { return (size_t)P.band_rows * P.W; }
__device__ __forceinline__ void dep_store(float4* base, size_t n, size_t off, float4 d) {
  float2* p = (float2*)base;
  p[off] = make_float2(d.x, d.y);
  p[n + off] = make_float2(d.z, d.w);
}
__device__ __forceinline__ float4 dep_load(const float4* base, size_t n, size_t off) {
  const float2* p = (const float2*)base;
  const float2 a = p[off], b = p[n + off];
  return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ float2 dep_load_xy(const float4* base, size_t off) { return ((const float2*)base)[off]; }
// Normals g-buffer slot layout: a [band_rows][W] plane of xyz (12 B per pixel) then a
// [band_rows][W] plane of w (the hit flag, 4 B).  The post-process's temporal test reads only
// the history normals' xyz (aop_postprocessing.glsl:180), 12 B per history slot instead of 16;
// the pixel itself and its neighbours read both planes.  rt_download / rt_upload_gbuffer convert
// to the reference's vec4 layout.
// (RT_NRM_PLANES=0: interleaved float4, the round-2 layout, for A/B builds)
__device__ __forceinline__ void nrm_store(float4* base, size_t n, size_t off, float4 v) {
  if (!RT_NRM_PLANES) {
    base[off] = v;
    return;
  }
  float* p = (float*)base;
  p[3 * off] = v.x;
  p[3 * off + 1] = v.y;
  p[3 * off + 2] = v.z;
  p[3 * n + off] = v.w;
}
__device__ __forceinline__ f3 nrm_load_xyz(const float4* base, size_t off) {
  if (!RT_NRM_PLANES) return xyz(base[off]);
  const float* p = (const float*)base;
  return mk(p[3 * off], p[3 * off + 1], p[3 * off + 2]);
}
__device__ __forceinline__ float nrm_load_w(const float4* base, size_t n, size_t off) {
  if (!RT_NRM_PLANES) return base[off].w;
  return ((const float*)base)[3 * n + off];
}
__device__ __forceinline__ float4 nrm_load(const float4* base, size_t n, size_t off) {
  const f3 v = nrm_load_xyz(base, off);
  return make_float4(v.x, v.y, v.z, nrm_load_w(base, n, off));
}

struct FrameDst {
  f3 light;
  float4* out_pix;
  float4* image;
};
// MF = false: a single-frame launch (mf_n = 0, the host's choice): the frame's light and
// destinations come straight from the kernel arguments, with no branch on mf_n, so a wave's
// first scalar loads issue together instead of one dependent round trip after another
template <bool MF = true>
__device__ __forceinline__ FrameDst frame_dst(const FrameParams& P, int j) {
  if (!MF || P.mf_n <= 0) return FrameDst{mk(P.Lx, P.Ly, P.Lz), P.out_pix, P.image};
  const float4 L = P.mf_light[j];
  return FrameDst{mk(L.x, L.y, L.z), (float4*)P.hist_pix[(P.mf_slot0 + j) % P.F], j == P.mf_n - 1 ? P.image : nullptr};
}
// The g-buffer slot a Phong/hybrid frame writes with rt_set_phong_gbuffer on (include/rt/abi.h
// "Phong g-buffer"; the GB instantiations only): the launch's slot, or frame j's of a batch.
struct GbDst {
  float4* nrm;
  float4* dep;
};
template <bool MF>
__device__ __forceinline__ GbDst frame_gb(const FrameParams& P, int j) {
  if (!MF || P.mf_n <= 0) return GbDst{P.nrm, P.dep};
  const int slot = (P.mf_slot0 + j) % P.F;
  return GbDst{(float4*)P.hist_nrm[slot], (float4*)P.hist_dep[slot]};
}
// The primary hit as the kernel found it: (n, 1) and (t, 0, 0, 1), or zeros for a miss; the colour
// store's lane-to-pixel map (store_color), the AO pass's plane layouts.  Plain stores, as the AO
// pass's: they keep the lines in the XCD's L2 for a post-process pass that may read them next.
__device__ __forceinline__ void store_gbuf(const FrameParams& P, const GbDst& gb, int x, int y, bool hit, f3 n, float t) {
  const size_t off = (size_t)(y - P.band_row0) * P.W + x;
  const float f = hit ? 1.0f : 0.0f;
  nrm_store(gb.nrm, dep_plane(P), off, hit ? make_float4(n.x, n.y, n.z, f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  dep_store(gb.dep, dep_plane(P), off, make_float4(hit ? t : 0.0f, 0.0f, 0.0f, f));
}

// Multi-frame launches of modes 3/4 (FrameParams::mf_n frames): each block renders its tile in
// frames blockIdx.z * FPB ... (up to FPB of them, one after another), so a launch dispatches FPB x
// fewer workgroups and stages its LDS tables once per tile, not once per frame.  Every frame's
// tile is traced and shaded in full.  Phong (config (a), short waves bound by the workgroup
// dispatch rate): FPB 4, +5% over 1 (2: +3%, 8: +0%); hybrid (config (b)): 1 (2: -1.3%,
// 4: -2.7%, 8: -17%; its waves are longer and the mirror bounces of a few tiles set the tail)
// (tools/explore/r02m.sh).
constexpr int kPhongFramesPerBlock = 4, kHybridFramesPerBlock = 1;

template <int FPB>
__device__ __forceinline__ int block_frames(const FrameParams& P, int& j0) {
  if (P.mf_n <= 0) {
    j0 = 0;
    return 1;
  }
  j0 = (int)blockIdx.z * FPB;
  return P.mf_n - j0 < FPB ? P.mf_n - j0 : FPB;
}

// ---------------------------------------------------------------------------------------
// Primary-ray cone culling (used by ao_batch_kernel, phong_kernel, hybrid_kernel).  Every primary ray starts at the camera
// and passes through the pool's pixel rectangle (jitter < 0.0834 px), so one cone bounds
// them.  A sphere whose line distance from every ray of the cone exceeds its radius by a
// float-error margin has a computed discriminant < 0 for every lane (-1 in the reference,
// never accepted) and is skipped.
// ---------------------------------------------------------------------------------------
constexpr float kInv6 = 1.0f / 6.0f;  // correctly rounded (div_rn_by)
constexpr int kPool = kAoPool;
constexpr int kSetupCost = 24;
constexpr int kTailMaxObj = 128;  // split tail rounds stage the sphere table in LDS up to this size  // per-sample setup (hashes, directions, shading) in sphere-test units

// Float form of the same cull (no trig): cone axis a, cos/sin of the half-angle; a sphere
// with inflated radius r_eff (r_eff^2 = r^2 + 1e-5 (d^2 + r^2)) lies outside the forward and
// the backward cone iff |cos phi| < cos(theta + alpha), sin alpha = r_eff / d.  Float error
// (~1e-6) is covered by the 2e-5 slack on the cosine and the 1e-5 inflation.
// threadIdx.x & 63 recomputed at the point of use (volatile: not hoisted or shared)
__device__ __forceinline__ int lane_id_here() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

struct ConeF {
  float ax, ay, az, ct, st;
};

// The cone only has to be conservative, not bit-exact: it is built with the raw
// v_rcp/v_sqrt/v_rsq instructions (<= 1 ulp, ~1e-7 relative), far inside the 2e-5 cosine
// slack and the 1e-5 radius inflation.
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }

__device__ inline ConeF pool_cone_f(const FrameParams& P, int xmin, int xmax, int ymin, int ymax) {
  const float iw = fast_rcp(P.fW), ih = fast_rcp(P.fH);
  const float hps[2] = {((float)xmin - 0.1f) * iw, ((float)xmax + 0.1f) * iw};
  const float vps[2] = {((float)ymin - 0.1f) * ih, ((float)ymax + 0.1f) * ih};
  f3 d[4];
  f3 sum = mk(0.0f, 0.0f, 0.0f);
  for (int k = 0; k < 4; ++k) {
    float hp = hps[k & 1], vp = vps[k >> 1];
    f3 v = mk(P.lx + hp * P.hx + vp * P.vx, P.ly + hp * P.hy + vp * P.vy, P.lz + hp * P.hz + vp * P.vz);
    d[k] = fast_rsq(dot(v, v)) * v;
    sum = sum + d[k];
  }
  const float il = fast_rsq(dot(sum, sum));
  ConeF c;
  c.ax = sum.x * il; c.ay = sum.y * il; c.az = sum.z * il;
  float ct = 1.0f;
  for (int k = 0; k < 4; ++k) ct = fminf(ct, c.ax * d[k].x + c.ay * d[k].y + c.az * d[k].z);
  ct = fminf(fmaxf(ct - 2e-5f, -1.0f), 1.0f);  // widen the cone a little (direction rounding)
  c.ct = ct;
  c.st = fast_sqrt(fmaxf(0.0f, 1.0f - ct * ct));
  return c;
}

__device__ inline bool cone_misses_f(const ConeF& c, float4 g, float cx, float cy, float cz) {
  float Lx = g.x - cx, Ly = g.y - cy, Lz = g.z - cz;
  float d2 = Lx * Lx + Ly * Ly + Lz * Lz, r2 = g.w * g.w;
  float reff2 = r2 + 1e-5f * (d2 + r2);
  if (!(d2 > reff2 * 1.01f + 1e-6f)) return false;  // camera inside / near the sphere: keep
  float id = fast_rsq(d2);
  float sa2 = reff2 * (id * id);
  float sa = fast_sqrt(sa2), ca = fast_sqrt(fmaxf(0.0f, 1.0f - sa2));
  float K = c.ct * ca - c.st * sa - 2e-5f;  // cos(theta + alpha), made smaller (conservative)
  if (!(K > 0.0f)) return false;
  float cphi = (c.ax * Lx + c.ay * Ly + c.az * Lz) * id;
  return fabsf(cphi) < K;
}

// First-bounce cone of a prepared batch (ao_batch_kernel).  The live lanes' bounce rays start
// at primary hit points of the batch's few pixels and go into a hemisphere about the hit
// normal (or around the mirror direction), so their origins lie in a small ball (centre o,
// radius rho) and their directions in a cone (axis a, half-angle theta).  A sphere is skipped
// for the whole batch when, for every such ray, the reference's test provably rejects it:
//  (1) every origin is clearly outside the sphere: |c - o| - rho - r > 1e-2 (|c - o| + rho);
//  (2) the forward cone from o misses the sphere inflated to r_eff + rho, r_eff^2 = r^2 +
//      1e-5 (Lmax^2 + r^2): beta > theta + alpha with sin alpha = (r_eff + rho) / |c - o|.
// A ray from p (|p - o| <= rho) that met B(c, r_eff) would give the ray from o with the same
// direction a point within rho of it, so by (2) every ray's forward half-line misses
// B(c, r_eff).  If its closest approach to c lies ahead, the line passes at distance >= r_eff
// and the exact discriminant is <= -1e-5 (Lmax^2 + r^2), > 10x the computed-discriminant
// error (~7e-7 Lmax^2): the computed del is < 0 (-1, never accepted).  If it lies behind, both
// real roots are negative and, by (1), the larger one is below -(|p - c| - r) <= -1e-2 Lmax,
// > 10x the computed-root error (sqrt of the del error, ~8.4e-4 Lmax): the computed roots are
// negative, never above the 1e-4 threshold.  NaN anywhere fails a comparison and keeps the
// sphere.  Must be called by every lane of the wave.
struct ConeB {
  float ox, oy, oz, rho, ax, ay, az, ct, st;
};

__device__ __forceinline__ ConeB bounce_cone(bool live, f3 p, f3 d, unsigned long long lm) {
  ConeB c;
  const int first = __builtin_ctzll(lm);
  c.ox = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.x), first));
  c.oy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.y), first));
  c.oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.z), first));
  const float ex = p.x - c.ox, ey = p.y - c.oy, ez = p.z - c.oz;
  const float e2 = wave_max_f(live ? ex * ex + ey * ey + ez * ez : 0.0f);
  const float sx = wave_sum_f(live ? d.x : 0.0f), sy = wave_sum_f(live ? d.y : 0.0f), sz = wave_sum_f(live ? d.z : 0.0f);
  c.rho = fast_sqrt(e2) * 1.0001f + 1e-6f * (fabsf(c.ox) + fabsf(c.oy) + fabsf(c.oz));
  const float s2 = sx * sx + sy * sy + sz * sz;
  const float il = fast_rsq(s2);
  c.ax = sx * il; c.ay = sy * il; c.az = sz * il;
  float ct = wave_min_f(live ? c.ax * d.x + c.ay * d.y + c.az * d.z : 1.0f) - 2e-5f;
  if (!(s2 > 1e-6f)) ct = -1.0f;  // directions cancel: no usable axis
  ct = fminf(fmaxf(ct, -1.0f), 1.0f);
  c.ct = ct;
  c.st = fast_sqrt(fmaxf(0.0f, 1.0f - ct * ct));
  return c;
}

__device__ __forceinline__ bool bounce_cone_misses(const ConeB& c, float4 g) {
  const float vx = g.x - c.ox, vy = g.y - c.oy, vz = g.z - c.oz;
  const float L = fast_sqrt(vx * vx + vy * vy + vz * vz);
  const float r = fabsf(g.w), Lmax = L + c.rho;
  if (!((L - c.rho - r) > 1e-2f * Lmax)) return false;  // (1)
  const float R = fast_sqrt(r * r + 1e-5f * (Lmax * Lmax + r * r)) * 1.00001f + c.rho;
  const float sa = R * fast_rcp(L), ca = fast_sqrt(fmaxf(0.0f, 1.0f - sa * sa));
  if (!(c.st * ca + c.ct * sa > 1e-5f)) return false;  // theta + alpha >= pi: the cone covers the sphere
  const float K = c.ct * ca - c.st * sa - 2e-5f;         // cos(theta + alpha), made smaller
  const float cphi = (c.ax * vx + c.ay * vy + c.az * vz) * fast_rcp(L);
  return cphi < K;  // (2)
}

// bounce_cone_misses plus the sphere's per-ray pre-test for the batch: with theta = 0 (the
// cone of ONE ray, around its own direction d) the same argument shows that a live lane
// whose direction has dot(d, (c - o) / |c - o|) < cos(alpha) - 2e-5 cannot accept the sphere
// (|d| = 1 within 3e-7 and u's fast-math error is ~1e-7, both far inside the 2e-5 slack).
// pt = (u, K) with K = cos(alpha) - 2e-5, or K = -2 (every lane tests) when (1) fails.
__device__ __forceinline__ bool bounce_cone_keep_pt(const ConeB& c, float4 g, float4& pt) {
  const float vx = g.x - c.ox, vy = g.y - c.oy, vz = g.z - c.oz;
  const float L = fast_sqrt(vx * vx + vy * vy + vz * vz);
  const float r = fabsf(g.w), Lmax = L + c.rho;
  pt = make_float4(0.0f, 0.0f, 0.0f, -2.0f);
  if (!((L - c.rho - r) > 1e-2f * Lmax)) return true;  // (1)
  const float R = fast_sqrt(r * r + 1e-5f * (Lmax * Lmax + r * r)) * 1.00001f + c.rho;
  const float il = fast_rcp(L);
  const float sa = R * il, ca = fast_sqrt(fmaxf(0.0f, 1.0f - sa * sa));
  const float ux = vx * il, uy = vy * il, uz = vz * il;
  if (sa < 1.0f) pt = make_float4(ux, uy, uz, ca - 2e-5f);
  if (!(c.st * ca + c.ct * sa > 1e-5f)) return true;
  const float K = c.ct * ca - c.st * sa - 2e-5f;
  const float cphi = c.ax * ux + c.ay * uy + c.az * uz;
  return !(cphi < K);  // (2)
}

// Bounce-ray cluster cull (ao_batch_kernel's later bounce rounds).  A cluster cb = (centre, R)
// holds spheres with |c_i - centre| + |r_i| <= R (rt_shim build_clusters).  The ray (p, d), |d|
// = 1 within 3e-7, provably accepts none of them when
//  (A) its line passes the centre at distance h > R' = R + 0.0032 (Lmax + R), Lmax = |p - centre|
//      + R >= |p - c_i|: then every member's line distance is h_i > r_i + sqrt(1e-5 (d_i^2 +
//      r_i^2)) >= r_eff (the cone culls' inflated radius, d_i = |p - c_i|), so the exact
//      discriminant is <= -1e-5 (d_i^2 + r_i^2), > 5x the computed one's float error:
//      the computed del is < 0 (-1 in the reference, never accepted).  The computed h^2 =
//      fmaf(-b, b, L2) is within ~1.3e-6 L2 of the exact one, covered by the 4e-6 L2 slack;
//  (B) or the ball lies behind the origin (d . (centre - p) < -R' - 1e-3 (u + R')) while the
//      origin is outside it (u - R' > 1e-2 (u + R'), u = |p - centre|): for every member the
//      closest approach is behind (b_i > 0 with margin) and the origin is outside it by more than
//      1e-2 (|p - c_i| + r_i), so both roots are negative by more than 10x the computed-root error
//      (bounce_cone_misses (1)): never above the 1e-4 threshold.
// NaN anywhere fails both tests and keeps the cluster.
#ifndef RT_CLUSTER_TAIL_MAX_G
#define RT_CLUSTER_TAIL_MAX_G 8
#endif
constexpr int kClusterTailMaxG = RT_CLUSTER_TAIL_MAX_G;  // split tail rounds with G <= this use the cluster cull
__device__ __forceinline__ bool cluster_may_hit(f3 p, f3 d, float4 cb) {
  const float vx = cb.x - p.x, vy = cb.y - p.y, vz = cb.z - p.z;
  const float L2 = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
  const float b = fmaf(d.z, vz, fmaf(d.y, vy, d.x * vx));  // > 0: the centre lies ahead
  const float u = fast_sqrt(L2);
  const float Rp = fmaf(0.0032f, u + 2.0f * cb.w, cb.w);
  const bool line_miss = fmaf(-b, b, L2) > fmaf(Rp, Rp, 4e-6f * L2);
  const bool behind = (b + Rp) < -1e-3f * (u + Rp) && (u - Rp) > 1e-2f * (u + Rp);
  return !(line_miss || behind);
}
// The wave mask of the lanes (full exec mask) whose ray may hit the cluster: cluster_may_hit as
// three ballots of single compares, !line_miss & (!c1 | !c2), each a negated compare that is true
// on NaN (so NaN keeps the cluster, as above).  The compiler's ballot of the combined bool went
// through a v_cndmask + v_cmp pair per cluster.
__device__ __forceinline__ unsigned long long cluster_may_hit_mask(f3 p, f3 d, float4 cb) {
  const float vx = cb.x - p.x, vy = cb.y - p.y, vz = cb.z - p.z;
  const float L2 = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
  const float b = fmaf(d.z, vz, fmaf(d.y, vy, d.x * vx));
  const float u = fast_sqrt(L2);
  const float Rp = fmaf(0.0032f, u + 2.0f * cb.w, cb.w);
  const unsigned long long nlm = __builtin_amdgcn_ballot_w64(!(fmaf(-b, b, L2) > fmaf(Rp, Rp, 4e-6f * L2)));
  const unsigned long long nc1 = __builtin_amdgcn_ballot_w64(!((b + Rp) < -1e-3f * (u + Rp)));
  const unsigned long long nc2 = __builtin_amdgcn_ballot_w64(!((u - Rp) > 1e-2f * (u + Rp)));
  return nlm & (nc1 | nc2);
}

// ---- the query tree's device functions (the kernels: "The query tree" below; here, ahead of the
// self-test kernel, which runs them alone as RT_MATH_CULL_TREE) ----
// The unit gate.  cluster_may_hit's proof takes a direction with | |d| - 1 | <= 3e-7, and
// rt_trace_rays takes d as given, so a lane culls only when s = dot(d, d), the fused chain, has
// |s - 1| <= kUnitGate.  s - 1 is exact (Sterbenz) and a multiple of 2^-24 below 1, of 2^-23 above,
// so the gate admits s in [1 - 7 * 2^-24, 1 + 3 * 2^-23] = [1 - 4.1724e-7, 1 + 3.5763e-7].  The
// chain rounds three times, each partial sum at most the total: |s - E| <= 3 * 2^-24 E (1 + 2^-24)^2
// < 1.7882e-7 for the exact E = |d|^2 <= 1 + 6e-7.  Hence E in [1 - 5.9606e-7, 1 + 5.3645e-7] and
// |d| = sqrt(E) in [1 - 2.9804e-7, 1 + 2.6823e-7], inside the proof's 3e-7.  A direction that fails
// (NaN included: the comparison is false) keeps every ball, so its lane visits every leaf and gets
// the linear scan's answer.  normalize()'s outputs pass: over 4 * 10^7 random vectors s stayed in
// [1 - 6 * 2^-24, 1 + 3 * 2^-23] (and tests/test_gpu_query_tree.py holds it on the device).
constexpr float kUnitGate = 4.2e-7f;
__device__ __forceinline__ bool unit_gate(f3 d) { return fabsf(dot(d, d) - 1.0f) <= kUnitGate; }
// A node's decision: cluster_may_hit itself (NaN keeps the node), for a lane that passed the gate.
__device__ __forceinline__ bool tree_may_hit(bool gate, f3 o, f3 d, float4 cb) { return !gate || cluster_may_hit(o, d, cb); }

// One sphere of the tree's closest-hit walk: query_sphere's value arithmetic (the same dot, fmaf
// discriminant, sqrt_rn, root selection and del == 0 case) per lane, without its wave-uniform ballot
// branch (the sphere differs from lane to lane here), merged by planar_candidate's order-free rule:
// the accepted candidate of least t and, among equal t, least index, which is what the ascending
// scan with its strict '<' ends with.
__device__ __forceinline__ void tree_sphere(f3 pos, f3 dir, float4 g, int i, float thr, float& t, int& ind) {
  const f3 pmc = pos - xyz(g);
  const float b = dot(dir, pmc);
  const float del = fmaf(g.w, g.w, fmaf(b, b, -dot(pmc, pmc)));
  const float s = sqrt_rn(del);
  const float nb = -1.0f * b;
  const float t1 = nb + s, t2 = nb - s;
  float res = (t2 < 0.0f) ? ((t1 < 0.0f) ? -1.0f : t1) : t2;
  res = (del == 0.0f) ? nb : res;
  const bool acc = (del >= 0.0f) & (res > thr) & ((t < 0.0f) | (res < t) | ((res == t) & (i < ind)));
  t = acc ? res : t;
  ind = acc ? i : ind;
}

// ---------------------------------------------------------------------------------------
// Planes (plane_eval_ray, p_compute.glsl:111-119) in the cone-culled kernels.  The spheres
// keep their culled, ascending scan over the sphere table (P.sph: planes and every other
// shape are NaN there, never accepted); the planes are tested after it from the compact plane
// table and merged by plane_candidate's lexicographic (t, index) rule, which is the result of
// the reference's ascending scan whatever the visiting order.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long uniform_mask(unsigned long long m) {
  return ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((unsigned)m);
}

// every plane of the scene (RC: every entry of the plane table, rectangles in effect among them)
template <bool RC = false>
__device__ __forceinline__ void plane_pass(const FrameParams& P, f3 pos, f3 dir, float thr, float& t, int& ind) {
  for (int k = 0; k < P.nplanes; ++k)
    planar_candidate<RC>(P.planes, pos, dir, P.planes[2 * k], P.planes[2 * k + 1], thr, t, ind);
}

// the planes k < 64 whose bit is set in the wave-uniform mask m, and every plane k >= 64
template <bool RC = false>
__device__ __forceinline__ void plane_pass_masked(const FrameParams& P, unsigned long long m, f3 pos, f3 dir, float thr,
                                                  float& t, int& ind) {
  while (m) {
    const int k = __builtin_ctzll(m);
    m &= m - 1;
    planar_candidate<RC>(P.planes, pos, dir, P.planes[2 * k], P.planes[2 * k + 1], thr, t, ind);
  }
  for (int k = 64; k < P.nplanes; ++k)
    planar_candidate<RC>(P.planes, pos, dir, P.planes[2 * k], P.planes[2 * k + 1], thr, t, ind);
}

// A plane that no camera ray of the cone can accept.  Every such ray starts at the camera, so
// its numerator dot(n, p0 - cam) is the same float on every lane (computed here by the same
// operations).  The ray's t = num / denom is accepted only if denom has num's sign and is
// outside (-0.001, 0.001); the denominators dot(n, d) of the cone's directions lie within
// |n| [cos(min(phi + theta, pi)), cos(max(phi - theta, 0))], phi = angle(n, axis).  With a
// 1e-4 |n| slack (the cone's float error is ~1e-6; the lanes' dot error ~3e-7 |n|) a plane
// outside that window for its sign is missed by every lane (-1 or a value <= 0, never accepted).
// NaN fails every comparison and keeps the plane.
__device__ __forceinline__ bool plane_cone_misses(const ConeF& c, float4 a, float4 b, f3 cam) {
  const f3 n = xyz(a);
  const float num = dot(n, xyz(b) - cam);
  if (num == 0.0f) return true;  // res = +-0 (or NaN): never above a threshold >= 0
  const float n2 = n.x * n.x + n.y * n.y + n.z * n.z;
  if (n2 == 0.0f) return true;  // denom = 0: the parallel case, -1
  const float nl = fast_sqrt(n2);
  const float cphi = (c.ax * n.x + c.ay * n.y + c.az * n.z) * fast_rcp(nl);
  const float sphi = fast_sqrt(fmaxf(0.0f, 1.0f - cphi * cphi));
  if (num > 0.0f) {  // accepted only with denom >= 0.001
    const float cmax = cphi > c.ct ? 1.0f : cphi * c.ct + sphi * c.st;
    return nl * (cmax + 1e-4f) < 0.001f;
  }
  if (num < 0.0f) {  // accepted only with denom <= -0.001
    const float cmin = cphi < -c.ct ? -1.0f : cphi * c.ct - sphi * c.st;
    return nl * (cmin - 1e-4f) > -0.001f;
  }
  return false;  // NaN
}

// wave-uniform mask of the planes k < 64 that the cone does not exclude (a rectangle's entry is
// tested as its plane: a cone that cannot reach the plane cannot reach a part of it)
__device__ __forceinline__ unsigned long long plane_cone_mask(const FrameParams& P, const ConeF& cone, f3 cam) {
  const int k = lane_id_here();
  const bool keep = k < P.nplanes && !plane_cone_misses(cone, P.planes[2 * k], P.planes[2 * k + 1], cam);
  return uniform_mask(__ballot(keep));
}

// Closest hit of the camera rays of a pixel rectangle whose cone is `cone`: per 64-sphere
// word the wave culls the spheres lane-parallel, then tests the survivors in ascending index
// order, reading them on the scalar path (wave-uniform index).  PL: then the planes the cone
// does not exclude.  Same result as closest_hit.  Must be called by every lane of the wave.
// SKIP (timing ablation): cull only, no tests.
// Camera rays only: every ray starts at the header's camera (P.cx, P.cy, P.cz).  The survivors are
// tested from the per-frame camera-relative rows (P.camrel: camera - centre and its self dot,
// computed on the host with the same float operations), so each test skips the three subtractions
// and the self dot; rays from any other origin must use closest_hit / closest_hit_pf.
template <bool PL, bool SKIP = false, bool RC = false>
__device__ __forceinline__ int closest_hit_cone(const FrameParams& P, const float4* __restrict__ geo, int nobj,
                                                const ConeF& cone, f3 dir, float thr, float& t_out,
                                                const float4* pre0 = nullptr) {
  float t = -1.0f;
  int ind = -1;
  const int lane = threadIdx.x & 63;
  const f3 cam = mk(P.cx, P.cy, P.cz);
  const float4* const cr = P.camrel;
  auto word = [&](int w, bool keep) {
    unsigned long long m = uniform_mask(__ballot(keep));
    const float4* const gw = geo + w;  // (unsigned row offset: one scalar shift per survivor)
    const float4* const cw = cr + w;
    while (m && !SKIP) {
      const unsigned j = (unsigned)pop_lowest(m);
      sphere_candidate_rel(dir, cw[j], gw[j].w, w + (int)j, thr, t, ind);
    }
  };
  int w = 0;
  if (pre0 && nobj > 0) {  // the first word's rows, already requested by the caller
    word(0, lane < nobj && !cone_misses_f(cone, *pre0, cam.x, cam.y, cam.z));
    w = 64;
  }
  for (; w < nobj; w += 64) {
    const int i = w + lane;
    word(w, i < nobj && !cone_misses_f(cone, geo[i], cam.x, cam.y, cam.z));
  }
  if (PL) plane_pass_masked<RC>(P, plane_cone_mask(P, cone, cam), cam, dir, thr, t, ind);
  t_out = t;
  return ind;
}

// The cone of the camera rays through this wave's 8x8 pixel tile (tile_xy of tile (bx, by)).
template <int BWX = 2, int BWY = 2>
__device__ __forceinline__ ConeF wave_tile_cone(const FrameParams& P, int bx, int by) {
  const int wave = threadIdx.x >> 6;
  const int x0 = bx * 8 * BWX + (wave % BWX) * 8, y0 = P.trace_row0 + by * 8 * BWY + (wave / BWX) * 8;
  return pool_cone_f(P, x0, x0 + 7, y0, y0 + 7);
}

// shadow_ray (p_compute.glsl:145-166) for the whole wave at once, all-sphere scenes: every
// shadow line passes (within ~3e-5) through the light, so the lines of the lanes that need
// one lie in a cone with its apex at the light.  Spheres outside that cone (radius inflated
// for the longest line's rounding and by 1e-4, shadow_cone_keeps, plus cone_misses_f's margins)
// are missed by every line (-1, never an occluder); the
// rest are tested as shadow_lit does.  "Some occluder exists" does not depend on the order.
// Must be called by every lane of the wave (ballots and shuffles).
#ifndef RT_SHADOW_CONE_MIN
#define RT_SHADOW_CONE_MIN 8
#endif
constexpr int kShadowConeMinObj = RT_SHADOW_CONE_MIN;
// the binary64 occluder test of shadow_ray (p_compute.glsl:155-163) for one object's float t:
// t > 0.0001 and length(dvec3(t * l)) < len, the binary64 sequence for every such t
__device__ __forceinline__ bool shadow_occludes(float tf, f3 l, double dlen) {
  if (!(tf > 0.0001f)) return false;  // (double)tf > (double)0.0001f, exactly
  const double t = (double)tf;
  const double dx = t * (double)l.x, dy = t * (double)l.y, dz = t * (double)l.z;
  return sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) < dlen;
}
// The cone at the light over the directions -l of the lanes that need a shadow ray (DPP
// reductions; the cone only has to contain every lane's direction, whatever the sum order), and
// lmax, the longest of their lines (len = |light - pos|).  Must be called by every lane of the wave.
__device__ __forceinline__ ConeF shadow_cone(bool need, f3 l, float len, float& lmax) {
  lmax = wave_max_f(need ? len : 0.0f);
  const float sx = wave_sum_f(need ? -l.x : 0.0f), sy = wave_sum_f(need ? -l.y : 0.0f),
              sz = wave_sum_f(need ? -l.z : 0.0f);
  const float il = __builtin_amdgcn_rsqf(sx * sx + sy * sy + sz * sz);
  ConeF cone;
  cone.ax = sx * il; cone.ay = sy * il; cone.az = sz * il;
  float cd = wave_min_f(need ? -(cone.ax * l.x + cone.ay * l.y + cone.az * l.z) : 1.0f);
  cd = fminf(fmaxf(cd - 2e-5f, -1.0f), 1.0f);
  cone.ct = cd;
  cone.st = __builtin_amdgcn_sqrtf(fmaxf(0.0f, 1.0f - cd * cd));
  return cone;
}
// A sphere row that the shadow cone does not exclude (wide: the cone is nearly a half-space).
// A shadow ray starts at the shaded point, up to Lmax = lmax + |c - light| from the sphere's centre,
// and its computed discriminant errs by ~7e-7 Lmax^2 whatever the sphere's distance D from the
// light; cone_misses_f's own inflation, 1e-5 (D^2 + r^2), covers that for rays from the apex only.
// So the radius tested is r' = sqrt(r^2 + 1e-5 Lmax^2) (1 + 1e-5) + 1e-4: a line that passes at r'
// or more has an exact discriminant <= -1e-5 Lmax^2, 14x the error, as in bounce_cone_misses.  With
// D alone a small sphere next to the light was culled while the reference's own rounding reported it
// as the occluder of points 20 D and more away (tests/test_gpu_culls.py, the long-line cases).
__device__ __forceinline__ bool shadow_cone_keeps(const ConeF& cone, bool wide, float4 g, f3 light, float lmax) {
  const float vx = g.x - light.x, vy = g.y - light.y, vz = g.z - light.z;
  const float Lm = lmax + fast_sqrt(vx * vx + vy * vy + vz * vz);
  const float rr = fast_sqrt(g.w * g.w + 1e-5f * (Lm * Lm)) * 1.00001f + 1e-4f;
  return wide || !cone_misses_f(cone, make_float4(g.x, g.y, g.z, rr), light.x, light.y, light.z);
}
// PL: planes occlude too (any shape type does, p_compute.glsl:153); they are tested after the
// spheres ("some occluder exists" does not depend on the order).
template <bool PL, bool RC = false>
__device__ __forceinline__ bool shadow_lit_cone(const FrameParams& P, const float4* __restrict__ geo, int n, f3 light,
                                                f3 pos, bool need, const float4* pre0 = nullptr) {
  const f3 lv = light - pos;
  const f3 l = normalize(lv);
  const float len = sqrtf(dot(lv, lv));
  const f3 np = pos + 0.01f * l;
  const double dlen = (double)len;
  if (__ballot(need) == 0) return true;
  bool lit = true;
  if (PL)
    for (int k = 0; k < P.nplanes; ++k)
      if (need && lit && shadow_occludes(planar_eval<RC>(P.planes, np, l, P.planes[2 * k], P.planes[2 * k + 1]), l, dlen)) lit = false;
  if (n <= kShadowConeMinObj) {  // small scenes: the cone costs more than it saves
    for (int k = 0; k < n; ++k) {
      if (need && lit && shadow_occludes(sphere_eval_shadow(np, l, geo[k]), l, dlen)) lit = false;
    }
    return lit;
  }
  float lmax;
  const ConeF cone = shadow_cone(need, l, len, lmax);
  const bool wide = !(cone.ct > 0.05f);  // nearly a half-space: test everything
  const int lane = threadIdx.x & 63;
  auto word = [&](int w, bool keep) {
    unsigned long long m = uniform_mask(__ballot(keep));
    const float4* const gw = geo + w;
    while (m) {
      const unsigned j = (unsigned)pop_lowest(m);
      if (need && lit && shadow_occludes(sphere_eval_shadow(np, l, gw[j]), l, dlen)) lit = false;
    }
  };
  auto keep_row = [&](float4 g) { return shadow_cone_keeps(cone, wide, g, light, lmax); };
  int w = 0;
  if (pre0) {  // the first word's rows, already requested by the caller (n > kShadowConeMinObj here)
    word(0, lane < n && keep_row(*pre0));
    w = 64;
  }
  for (; w < n; w += 64) {
    const int i = w + lane;
    word(w, i < n && keep_row(geo[i]));
  }
  return lit;
}

// ---------------------------------------------------------------------------------------
// mode 3 — p_compute.glsl:168-245
// ---------------------------------------------------------------------------------------
// shadow_ray over the sphere table (every lane on its own; the hybrid kernel's bounces), with
// the planes first when the scene has some (any order: "some occluder exists")
template <bool PL, bool RC = false>
__device__ __forceinline__ bool shadow_lit_sph(const FrameParams& P, const float4* __restrict__ geo, int n, f3 light,
                                               f3 pos) {
  const f3 lv = light - pos;
  const f3 l = normalize(lv);
  const float len = sqrtf(dot(lv, lv));
  const f3 np = pos + 0.01f * l;
  const double dlen = (double)len;
  if (PL)
    for (int k = 0; k < P.nplanes; ++k)
      if (shadow_occludes(planar_eval<RC>(P.planes, np, l, P.planes[2 * k], P.planes[2 * k + 1]), l, dlen)) return false;
  for (int i = 0; i < n; ++i)
    if (shadow_occludes(sphere_eval_shadow(np, l, geo[i]), l, dlen)) return false;
  return true;
}

// The kernels below come in two families.  ALLSPH (production): the sphere table P.sph is
// read on the scalar path from global memory, the camera rays of each wave's 8x8 tile and
// their shadow rays are cone-culled, and PL adds the scene's planes (plane table, tested after
// the spheres).  !ALLSPH (A/B builds only): the whole shape table staged in LDS, every shape
// tested through eval_ray's id dispatch, no culling.
// GB: the pixel's primary hit goes to the g-buffer slot *gb as well (store_gbuf).
// RC (with ALLSPH and PL): the plane table may hold rectangles in effect (rt_device.h planar_eval).
template <bool ALLSPH, bool PL, bool LT, int BWX = 2, int BWY = 2, bool GB = false, bool RC = false>
__device__ __forceinline__ void phong_tile(const FrameParams& P, const float4* lds, int bx, int by, const FrameDst& fd,
                                           const float4* __restrict__ gsph, const float4* __restrict__ gshp,
                                           const float4* pre0 = nullptr, const GbDst* gb = nullptr) {
  const int n = P.nobj;
  const float4* tab = (ALLSPH && !LT) ? gshp : lds;                       // geo | geo2 | col
  const float4* geo = (ALLSPH && !LT) ? gsph : (ALLSPH ? lds + 4 * n : lds);  // what the sphere tests read
  const int stride = (ALLSPH && !LT) ? P.S : n;
  const float4 *geo2 = tab + stride, *col = tab + 2 * stride;
  int x, y;
  tile_xy<BWX, BWY>(x, y, P.trace_row0, bx, by);
  const bool active = x < P.W && y < P.trace_row0 + P.trace_rows;
  const f3 cam = mk(P.cx, P.cy, P.cz), light = fd.light;
  const f3 dir = primary_dir(P, div_rn_by((float)x, P.fW, P.inv_W), div_rn_by((float)y, P.fH, P.inv_H));
  float t;
  int ind;
  if (ALLSPH) {
    const ConeF cone = wave_tile_cone<BWX, BWY>(P, bx, by);
    ind = closest_hit_cone<PL, false, RC>(P, geo, n, cone, dir, 0.0f, t, pre0);
  } else {
    ind = closest_hit<ALLSPH>(geo, geo2, n, cam, dir, 0.0f, t);
  }
  count_work(P, active, y, 1u, active && ind != -1 ? 1u : 0u);
  const bool need = active && ind != -1;
  bool lit_w = true;
  if (ALLSPH) lit_w = shadow_lit_cone<PL, RC>(P, geo, n, light, cam + t * dir, need, pre0);  // every lane takes part
  if (!active) return;
  float r, g, b;
  if (ind == -1) {
    r = P.bg.x; g = P.bg.y; b = P.bg.z;
    if (GB) store_gbuf(P, *gb, x, y, false, mk(0.0f, 0.0f, 0.0f), 0.0f);
  } else {
    f3 curr = cam + t * dir;
    bool lit = ALLSPH ? lit_w : shadow_lit<ALLSPH>(geo, geo2, n, light, curr);
    int id = (ALLSPH && !PL) ? SHAPE_SPHERE : __float_as_int(geo2[ind].w);
    f3 nn = shape_normal_rc<RC>(tab[ind], id, curr);
    if (GB) store_gbuf(P, *gb, x, y, true, nn, t);
    float4 c = col[ind];
    if (lit) {
      f3 l = normalize(light - curr);
      float spec = pow500(gclamp(dot(normalize(l - dir), nn), 0.0f, 1.0f));
      float k = gclamp(dot(nn, l), 0.06f, 1.0f);
      r = c.x * k + spec; g = c.y * k + spec; b = c.z * k + spec;
    } else {
      r = c.x * 0.06f; g = c.y * 0.06f; b = c.z * 0.06f;
    }
  }
  // result_color = vec4(0) + phong(dir); gamma; w = 0
  store_color(P, fd.out_pix, fd.image, x, y, gamma_out(0.0f + r, 0.0f + g, 0.0f + b));
}

// LT (ALLSPH, scenes of at most kTabLdsMax objects): the block stages the shape tables and the
// sphere table in LDS once ([4][n] + [n] float4), so the culls, the survivors' tests, the shadow
// rays and the shading read LDS instead of making dependent global round trips, whose latency
// the few resident waves of these short kernels do not hide.
#ifndef RT_TAB_LDS_MAX
#define RT_TAB_LDS_MAX 128
#endif
constexpr int kTabLdsMax = RT_TAB_LDS_MAX;
__device__ __forceinline__ void stage_tables(const FrameParams& P, float4* lds) {
  const int n = P.nobj;
  stage_shapes(P, lds);
  for (int k = threadIdx.x; k < n; k += blockDim.x) lds[4 * n + k] = P.sph[k];
}

// (the sphere and shape tables lead the arguments: preloaded into SGPRs, as for hybrid_kernel)
template <bool ALLSPH, bool PL = false, bool LT = false, bool MF = true>
__global__ __launch_bounds__(kBlock) void phong_kernel(const float4* __restrict__ gsph, const float4* __restrict__ gshp,
                                                       FrameParams P) {
  extern __shared__ float4 lds[];
  if (!ALLSPH || LT) {
    if (LT) stage_tables(P, lds);
    else stage_shapes(P, lds);
    __syncthreads();
  }
  if constexpr (!MF) {  // single-frame launch (frame_dst<false>)
    // the lane's row of the first 64-sphere word, requested before anything else (in bounds for
    // any scene: the sphere table is followed by >= 64 rows of other tables, rt_kernels.h)
    const float4 g0 = gsph[threadIdx.x & 63];
    phong_tile<ALLSPH, PL, LT>(P, lds, blockIdx.x, blockIdx.y, frame_dst<false>(P, 0), gsph, gshp,
                               (ALLSPH && !LT) ? &g0 : nullptr);
    return;
  }
  int j0;
  const int nj = block_frames<kPhongFramesPerBlock>(P, j0);
#pragma unroll 1
  for (int j = 0; j < nj; ++j)
    phong_tile<ALLSPH, PL, LT>(P, lds, blockIdx.x, blockIdx.y, frame_dst(P, j0 + j), gsph, gshp);
}

// phong_kernel<true, PL, false, MF> that also writes the frame's normals and depth (the GB tile).
// An entry point of its own, so that phong_kernel's instantiations keep their names and code.
template <bool PL, bool MF>
__global__ __launch_bounds__(kBlock) void phong_gbuf_kernel(const float4* __restrict__ gsph, const float4* __restrict__ gshp,
                                                            FrameParams P) {
  if constexpr (!MF) {
    const float4 g0 = gsph[threadIdx.x & 63];  // as phong_kernel
    const GbDst gb = frame_gb<false>(P, 0);
    phong_tile<true, PL, false, 2, 2, true>(P, nullptr, blockIdx.x, blockIdx.y, frame_dst<false>(P, 0), gsph, gshp, &g0,
                                            &gb);
    return;
  }
  int j0;
  const int nj = block_frames<kPhongFramesPerBlock>(P, j0);
#pragma unroll 1
  for (int j = 0; j < nj; ++j) {
    const GbDst gb = frame_gb<true>(P, j0 + j);
    phong_tile<true, PL, false, 2, 2, true>(P, nullptr, blockIdx.x, blockIdx.y, frame_dst(P, j0 + j), gsph, gshp, nullptr,
                                            &gb);
  }
}

// phong_kernel<true, true, false, MF> (GB: phong_gbuf_kernel<true, MF>) over a plane table with
// rectangles in effect (the RC tile): entry points of their own, so the kernels above keep their
// names and code.
template <bool MF, bool GB>
__global__ __launch_bounds__(kBlock) void phong_rc_kernel(const float4* __restrict__ gsph, const float4* __restrict__ gshp,
                                                          FrameParams P) {
  if constexpr (!MF) {
    const float4 g0 = gsph[threadIdx.x & 63];  // as phong_kernel
    const GbDst gb = frame_gb<false>(P, 0);
    phong_tile<true, true, false, 2, 2, GB, true>(P, nullptr, blockIdx.x, blockIdx.y, frame_dst<false>(P, 0), gsph, gshp,
                                                  &g0, GB ? &gb : nullptr);
    return;
  }
  int j0;
  const int nj = block_frames<kPhongFramesPerBlock>(P, j0);
#pragma unroll 1
  for (int j = 0; j < nj; ++j) {
    const GbDst gb = frame_gb<true>(P, j0 + j);
    phong_tile<true, true, false, 2, 2, GB, true>(P, nullptr, blockIdx.x, blockIdx.y, frame_dst(P, j0 + j), gsph, gshp,
                                                  nullptr, GB ? &gb : nullptr);
  }
}

// ---------------------------------------------------------------------------------------
// mode 4 — h_compute.glsl:186-321
// ---------------------------------------------------------------------------------------
// Mirror bounces (segments >= 1) of the live paths of a wave, one segment per round.  Few
// paths bounce (~3% of the pixels at config (b)), so a round usually has a handful of live
// lanes; then each live path gets a group of G = 64 / 2^ceil(log2 L) lanes: lane p of the group
// tests spheres p, p+G, ... and the group merges the partial closest hits (minimum t, lowest
// index on ties: exactly the ascending scan of h_compute.glsl:121-139), and likewise splits the
// segment's shadow ray ("some occluder exists" is order-free, p_compute.glsl:145-166).  With
// more than 32 live paths every lane traces its own.  Returns (for the owner lanes) t, ind, lit.
// Must be called by every lane of the wave; perm: this wave's 64-int LDS slice.
template <bool PL, bool RC = false>
__device__ __forceinline__ void bounce_round(const FrameParams& P, const float4* __restrict__ geo, int n, f3 light,
                                             bool live, f3 pos, f3 dir, int* perm, float& t_out, int& ind_out,
                                             bool& lit_out) {
  const unsigned long long lm = __ballot(live);
  const int L = __popcll(lm);
  const int lane = threadIdx.x & 63;
  if (L > 32) {
    float t = -1.0f;
    int ind = -1;
    bool lit = true;
    if (live) {
      ind = closest_hit_pf(geo, n, pos, dir, 0.001f, t);
      if (PL) plane_pass<RC>(P, pos, dir, 0.001f, t, ind);
      if (ind != -1) lit = shadow_lit_sph<PL, RC>(P, geo, n, light, pos + t * dir);
    }
    t_out = t;
    ind_out = ind;
    lit_out = lit;
    return;
  }
  int c = 0;
  while ((1 << c) < L) ++c;
  const int G = 64 >> c;  // the largest power of 2 with G * L <= 64
  const int rk = __builtin_amdgcn_mbcnt_hi((unsigned)(lm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lm, 0u));
  if (live) perm[rk] = lane;
  __builtin_amdgcn_wave_barrier();
  const int g = lane / G, pl = lane - g * G;
  const bool act = g < L;
  const int owner = act ? perm[g] : lane;
  __builtin_amdgcn_wave_barrier();
  const f3 o = mk(__shfl(pos.x, owner), __shfl(pos.y, owner), __shfl(pos.z, owner));
  const f3 d = mk(__shfl(dir.x, owner), __shfl(dir.y, owner), __shfl(dir.z, owner));
  float t = -1.0f;
  int ind = -1;
  if (act)
    for (int i = pl; i < n; i += G) sphere_candidate(o, d, geo[i], i, 0.001f, t, ind);
  for (int m = 1; m < G; m <<= 1) {  // every lane of the group ends with the group's result
    const float tb = __shfl_xor(t, m);
    const int ib = __shfl_xor(ind, m);
    const bool take = ib >= 0 && (ind < 0 || tb < t || (tb == t && ib < ind));
    t = take ? tb : t;
    ind = take ? ib : ind;
  }
  if (PL && act) plane_pass<RC>(P, o, d, 0.001f, t, ind);  // same planes, same result on every group lane
  // the segment's shadow ray, split the same way (the owner's hit point, same float ops)
  bool occ = false;
  if (act && ind != -1) {
    const f3 curr = o + t * d;
    const f3 lv = light - curr;
    const f3 l = normalize(lv);
    const float len = sqrtf(dot(lv, lv));
    const f3 np = curr + 0.01f * l;
    const double dlen = (double)len;
    if (PL)
      for (int k = pl; k < P.nplanes && !occ; k += G)
        occ = shadow_occludes(planar_eval<RC>(P.planes, np, l, P.planes[2 * k], P.planes[2 * k + 1]), l, dlen);
    for (int i = pl; i < n && !occ; i += G) occ = shadow_occludes(sphere_eval_shadow(np, l, geo[i]), l, dlen);
  }
  unsigned oc = occ ? 1u : 0u;
  for (int m = 1; m < G; m <<= 1) oc |= (unsigned)__shfl_xor((int)oc, m);
  const int src = live ? rk * G : lane;
  t_out = __shfl(t, src);
  ind_out = __shfl(ind, src);
  lit_out = __shfl((int)oc, src) == 0;
}

// ABL (A/B builds only, timing ablations): 1 = no shadow rays, 2 = no scene tests at all,
// 3 = primary cull only, 5 = no bounce segments, 6 = bounces without the split rounds
// GB: segment 0's hit goes to the g-buffer slot *gb as well (store_gbuf), there and then, so that
// neither t0 nor the normal stays live across the bounce rounds.
// RC (with ALLSPH and PL): the plane table may hold rectangles in effect, as in phong_tile.
template <bool ALLSPH, bool PL, bool LT, int ABL = 0, int BWX = 2, int BWY = 2, bool GB = false, bool RC = false>
__device__ __forceinline__ void hybrid_tile(const FrameParams& P, const float4* lds, int* perm, int bx, int by,
                                            const FrameDst& fd, const float4* __restrict__ gsph,
                                            const float4* __restrict__ gshp, const float4* pre0 = nullptr,
                                            const GbDst* gb = nullptr) {
  const int n = P.nobj;  // !ALLSPH or LT: LDS tables (see phong_kernel)
  const float4* tab = (ALLSPH && !LT) ? gshp : lds;
  const float4* geo = (ALLSPH && !LT) ? gsph : (ALLSPH ? lds + 4 * n : lds);
  const int stride = (ALLSPH && !LT) ? P.S : n;
  const float4 *geo2 = tab + stride, *col = tab + 2 * stride, *aux = tab + 3 * stride;
  int x, y;
  tile_xy<BWX, BWY>(x, y, P.trace_row0, bx, by);
  const bool active = x < P.W && y < P.trace_row0 + P.trace_rows;
  const f3 light = fd.light;
  const unsigned long long tstart = ABL == 7 ? __builtin_amdgcn_s_memrealtime() : 0;
  f3 pos = mk(P.cx, P.cy, P.cz);
  f3 dir = primary_dir(P, div_rn_by((float)x, P.fW, P.inv_W), div_rn_by((float)y, P.fH, P.inv_H));
  float arefl = 0.0f;          // array[2].w
  float rr = 0, rg = 0, rb = 0;  // result_color.rgb
  float c = 0.0f;
  unsigned nseg = 0, nshadow = 0;
  // hybrid_helper's shading of one segment's hit (or miss) plus hybrid's accumulation
  // (h_compute.glsl:241-295); returns true when the path stops
  auto segment = [&](int seg, float t, int ind, bool lit) -> bool {
    ++nseg;
    nshadow += ind == -1 ? 0u : 1u;
    float ar, ag, ab;
    bool stop;
    if (ind == -1) {
      ar = P.bg.x; ag = P.bg.y; ab = P.bg.z;
      stop = true;
      if (GB && seg == 0 && active) store_gbuf(P, *gb, x, y, false, mk(0.0f, 0.0f, 0.0f), 0.0f);
    } else {
      // (ABL 9, timing ablation with ABL 5's single segment: the shading without its table loads)
      float4 att = ABL == 9 ? make_float4(0.5f, 0.5f, 0.5f, 0.0f) : col[ind];
      f3 curr = pos + t * dir;
      int id = (ALLSPH && !PL) ? SHAPE_SPHERE : __float_as_int(geo2[ind].w);
      f3 nn = ABL == 9 ? normalize(curr) : shape_normal_rc<RC>(tab[ind], id, curr);
      if (GB && seg == 0 && active) store_gbuf(P, *gb, x, y, true, nn, t);
      if (lit) {
        f3 l = normalize(light - curr);
        float spec = pow500(gclamp(dot(normalize(l - dir), nn), 0.0f, 1.0f));
        float k = gclamp(dot(nn, l), 0.06f, 1.0f);
        ar = att.x * k + spec; ag = att.y * k + spec; ab = att.z * k + spec;
      } else {
        ar = att.x * 0.06f; ag = att.y * 0.06f; ab = att.z * 0.06f;
      }
      float refl = ABL == 9 ? 0.0f : 1.0f - aux[ind].y;
      if (refl < 0.001f) {
        stop = true;
      } else {
        stop = false;
        float dn = dot(dir, nn);
        dir = normalize(mk(dir.x - 2.0f * (dn * nn.x), dir.y - 2.0f * (dn * nn.y),
                           dir.z - 2.0f * (dn * nn.z)));
        pos = curr;
        arefl = refl;
      }
    }
    if (seg == 0) {
      c = arefl;
      rr = ar; rg = ag; rb = ab;
    } else {
      float den = 1.0f + c;
      rr = (rr + c * ar) / den;
      rg = (rg + c * ag) / den;
      rb = (rb + c * ab) / den;
      c = c * arefl;
    }
    return stop;
  };
  if (ALLSPH) {
    // segment 0: the camera rays of the wave's 8x8 tile and their shadow rays, cone-culled
    float t0 = -1.0f;
    int ind0 = -1;
    bool lit0 = true;
    const ConeF cone = wave_tile_cone<BWX, BWY>(P, bx, by);
    if (ABL != 2) ind0 = closest_hit_cone<PL, ABL == 3, RC>(P, geo, n, cone, dir, 0.001f, t0, pre0);
    if (ABL == 0 || ABL >= 4) lit0 = shadow_lit_cone<PL, RC>(P, geo, n, light, pos + t0 * dir, active && ind0 != -1, pre0);  // every lane takes part
    bool live = active && !segment(0, t0, ind0, lit0);
    // segments 1 .. D-1: bounce rounds with the whole wave
    int rounds = 0;  // wave-uniform: the wave's cost beyond its camera rays (tile schedule)
    for (int seg = 1; seg < ((ABL == 5 || ABL == 9) ? 1 : P.D); ++seg) {
      if (__ballot(live) == 0) break;
      ++rounds;
      float t;
      int ind;
      bool lit = true;
      if (ABL == 6) {
        if (live) {
          ind = closest_hit_pf(geo, n, pos, dir, 0.001f, t);
          if (PL) plane_pass<RC>(P, pos, dir, 0.001f, t, ind);
          if (ind != -1) lit = shadow_lit_sph<PL, RC>(P, geo, n, light, pos + t * dir);
        }
      } else {
        bounce_round<PL, RC>(P, geo, n, light, live, pos, dir, perm, t, ind, lit);
      }
      if (live) live = !segment(seg, t, ind, lit);
    }
    if (P.tile_cost && (threadIdx.x & 63) == 0)  // (a vector store from lane 0)
      P.tile_cost[((unsigned)by * gridDim.x + (unsigned)bx) * (BWX * BWY) + (threadIdx.x >> 6)] = (unsigned)rounds;
  } else {
    for (int seg = 0; active && seg < P.D; ++seg) {  // helper depth D, D-1, ..., 1
      float t;
      const int ind = closest_hit<ALLSPH>(geo, geo2, n, pos, dir, 0.001f, t);
      const bool lit = ind == -1 || shadow_lit<ALLSPH>(geo, geo2, n, light, pos + t * dir);
      if (segment(seg, t, ind, lit)) break;
    }
  }
  count_work(P, active, y, nseg, nshadow);
  if (active) store_color(P, fd.out_pix, fd.image, x, y, gamma_out(0.0f + rr, 0.0f + rg, 0.0f + rb));
  if (ABL == 7) {  // per-wave timeline (tools/explore/wave_timeline.py): lane 0's pixel slot holds
    // (start, end) of the wave's s_memtime and its longest path in segments
    const unsigned mx = wave_max(active ? nseg : 0u);
    const unsigned long long tend = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0 && active)
      P.out_pix[(size_t)(y - P.band_row0) * P.W + x] =
          make_float4(__uint_as_float((unsigned)tstart), __uint_as_float((unsigned)tend), __uint_as_float(mx),
                      __uint_as_float((unsigned)(tstart >> 32)));
  }
}

// The schedule's order table and the sphere / shape tables lead the argument list: the build
// preloads the first kernel arguments into SGPRs (-mllvm -amdgpu-kernarg-preload-count, Makefile),
// so a wave's first loads (its tile, then the culls' sphere rows) need not wait for a kernarg load.
// (FrameParams, an aggregate, is never preloaded.)
template <bool ALLSPH, bool PL = false, bool LT = false, int ABL = 0, int BWX = 2, int BWY = 2, bool MF = true>
__global__ __launch_bounds__(64 * BWX * BWY) void hybrid_kernel(const unsigned* __restrict__ tord,
                                                                const float4* __restrict__ gsph,
                                                                const float4* __restrict__ gshp, unsigned gx,
                                                                FrameParams P) {
  extern __shared__ float4 lds[];
  __shared__ int hperm[64 * BWX * BWY];  // bounce_round's live-rank -> lane map, a slice per wave
  if (!ALLSPH || LT) {
    if (LT) stage_tables(P, lds);
    else stage_shapes(P, lds);
    __syncthreads();
  }
  if constexpr (kHybridFramesPerBlock == 1) {  // no frame loop (the loop form costs 3-4% at (b))
    // the host's tile schedule (longest first, from the previous frames' bounce rounds): the
    // few tiles whose mirror paths bounce for many rounds start early instead of setting the
    // launch's tail (config (b): 32.0 -> 25.4 us per frame with the reverse of row order, which
    // happens to put that scene's bouncing tiles first)
    // MF = false: the lane's row of the first 64-sphere word requested before the tile order (in
    // bounds for any scene: the sphere table is followed by >= 64 rows of other tables)
    const bool pre = !MF && ALLSPH && !LT;
    float4 g0;
    if (pre) g0 = gsph[threadIdx.x & 63];
    unsigned bx = blockIdx.x, by = blockIdx.y;
    if (tord) {
      const unsigned t = tord[blockIdx.x + blockIdx.y * gx];  // (gx = gridDim.x, a preloaded argument)
      bx = t & 0xffffu;
      by = t >> 16;
    }
    hybrid_tile<ALLSPH, PL, LT, ABL, BWX, BWY>(P, lds, hperm + 64 * (threadIdx.x >> 6), bx, by,
                                               frame_dst<MF>(P, blockIdx.z), gsph, gshp, pre ? &g0 : nullptr);
  } else {
    int j0;
    const int nj = block_frames<kHybridFramesPerBlock>(P, j0);
#pragma unroll 1
    for (int j = 0; j < nj; ++j)
      hybrid_tile<ALLSPH, PL, LT, ABL, BWX, BWY>(P, lds, hperm + 64 * (threadIdx.x >> 6), blockIdx.x, blockIdx.y,
                                                 frame_dst(P, j0 + j), gsph, gshp);
  }
}

// hybrid_kernel<true, PL, false, 0, kHyBW, kHyBW, MF> that also writes the frame's normals and depth
// (the GB tile); an entry point of its own, as phong_gbuf_kernel is.
template <bool PL, int BWX, int BWY, bool MF>
__global__ __launch_bounds__(64 * BWX * BWY) void hybrid_gbuf_kernel(const unsigned* __restrict__ tord,
                                                                     const float4* __restrict__ gsph,
                                                                     const float4* __restrict__ gshp, unsigned gx,
                                                                     FrameParams P) {
  static_assert(kHybridFramesPerBlock == 1, "one frame per block (hybrid_kernel's loop-free form)");
  __shared__ int hperm[64 * BWX * BWY];
  float4 g0;
  if (!MF) g0 = gsph[threadIdx.x & 63];  // as hybrid_kernel
  unsigned bx = blockIdx.x, by = blockIdx.y;
  if (tord) {
    const unsigned t = tord[blockIdx.x + blockIdx.y * gx];
    bx = t & 0xffffu;
    by = t >> 16;
  }
  const GbDst gb = frame_gb<MF>(P, blockIdx.z);
  hybrid_tile<true, PL, false, 0, BWX, BWY, true>(P, nullptr, hperm + 64 * (threadIdx.x >> 6), bx, by,
                                                  frame_dst<MF>(P, blockIdx.z), gsph, gshp, MF ? nullptr : &g0, &gb);
}

// hybrid_kernel<true, true, false, 0, BWX, BWY, MF> (GB: hybrid_gbuf_kernel<true, BWX, BWY, MF>) over a
// plane table with rectangles in effect (the RC tile); an entry point of its own, as phong_rc_kernel is.
template <int BWX, int BWY, bool MF, bool GB>
__global__ __launch_bounds__(64 * BWX * BWY) void hybrid_rc_kernel(const unsigned* __restrict__ tord,
                                                                   const float4* __restrict__ gsph,
                                                                   const float4* __restrict__ gshp, unsigned gx,
                                                                   FrameParams P) {
  static_assert(kHybridFramesPerBlock == 1, "one frame per block (hybrid_kernel's loop-free form)");
  __shared__ int hperm[64 * BWX * BWY];
  float4 g0;
  if (!MF) g0 = gsph[threadIdx.x & 63];  // as hybrid_kernel
  unsigned bx = blockIdx.x, by = blockIdx.y;
  if (tord) {
    const unsigned t = tord[blockIdx.x + blockIdx.y * gx];
    bx = t & 0xffffu;
    by = t >> 16;
  }
  const GbDst gb = frame_gb<MF>(P, blockIdx.z);
  hybrid_tile<true, true, false, 0, BWX, BWY, GB, true>(P, nullptr, hperm + 64 * (threadIdx.x >> 6), bx, by,
                                                        frame_dst<MF>(P, blockIdx.z), gsph, gshp, MF ? nullptr : &g0,
                                                        GB ? &gb : nullptr);
}

// ---------------------------------------------------------------------------------------
// modes 1/2 pass 1 — ao_compute.glsl:143-339 (aop_compute.glsl:141-336)
// lane = (pixel, sample); ppb = blockDim / spp pixels per block, consecutive in a row.
// ---------------------------------------------------------------------------------------
enum { PRIM_HIT = 0, PRIM_MISS = 1, PRIM_EMISSIVE = 2 };

// ---------------------------------------------------------------------------------------
// Pooled AO (production, all scenes).  One wave per workgroup owns a pool of kPool pixel-samples
// (TP = kPool/spp consecutive pixels x spp samples).  New samples are prepared 64 at a time
// with the whole wave active: primary direction + hemisphere vector + primary hit
// over the culled set + first-hit shading.  Samples whose path ended at the primary hit are
// final at once; the live post-primary states are kept in the lanes that prepared them and
// handed to idle lanes by ds_bpermute whenever lanes run out of work.  Bounce rounds then
// run with (nearly) all lanes live, and no per-sample setup runs at partial utilisation.
// ---------------------------------------------------------------------------------------
// waves per SIMD the production AO kernel is compiled for (its register budget: 7 -> 72 VGPRs)
#ifndef RT_AO_MINW
#define RT_AO_MINW 7
#endif
constexpr int kAoMinWaves = RT_AO_MINW;
// 1 = the pools' samples sorted by bounce direction (AoConfig::SORT) for the scenes ao_select picks
// (kB1SortMinObj); 0 = no SORT instantiation is compiled (the A/B build, make b1sort0)
#ifndef RT_B1_SORT
#define RT_B1_SORT 1
#endif

// Compile-time configuration of ao_batch_kernel<C>: the defaults.  A configuration derives from
// this struct (or from a production one, AoProd below) and overrides members by name.
struct AoConfig {
  static constexpr int SPPC = 0;       // spp as a constant (0: P.spp): constant LDS offsets and it / spp, fewer scalars
  static constexpr int DC = 0;         // the depth as a constant (0: P.D)
  static constexpr bool PL = false;    // the scene has planes: tested after the spheres of every segment, culled against the pool cone
  static constexpr bool RC = false;    // with PL: the plane table may hold rectangles in effect (rt_device.h planar_eval)
  static constexpr bool CLON = false;  // launched only with clusters (P.ncl > 0): the rounds' plain full scan is not compiled
  static constexpr bool CNT = true;    // the work counters (false: compiled out, timed launches pass none)
  static constexpr bool MF = false;    // frame blockIdx.y of a multi-frame mode-2 launch: its own rand_buffer and slots (FrameParams::mf_rb)
  static constexpr bool LAZY = true;   // the empty-frustum shortcut; hemi computed after the primary hit, for hits only
  static constexpr bool TAIL = false;  // split tail rounds (the pool's last <= 32 paths, a lane group each)
  static constexpr bool B1 = false;    // a prepared batch's live paths take their first bounce together (bounce_cone)
  static constexpr bool PT = false;    // with B1: the per-ray pre-test of the cone's survivors, rows in LDS; with TAIL: its sphere table in LDS
  static constexpr bool PTW = false;   // with PT, above kTailMaxObj spheres: pre-test rows one 64-sphere word at a time, tail rounds
                                       // on the global table, rand_buffer read from global memory (no LDS copy)
  // The pool's samples dealt to its 64-lane batches by bounce direction instead of in item order:
  // the batches then each cover about a quarter of the hemisphere and the batched first bounce's
  // cone keeps fewer spheres (tools/explore/b1_sort_sim.py).  Before the first batch the wave
  // computes hemi = get_pt_within_unit_sphere for all of the pool's samples (it depends on (aa,
  // pixel, rand_buffer) only), parks it in the sample's three sres slots (free until finish(it);
  // prepare() reads it back first), and counting-sorts the items by hemi's octant, the 8 bins in
  // Gray-code order, item order inside a bin: order[slot] = item.  Every sample's path is a
  // function of its item only and the cone, cull and pre-test are conservative filters visited in
  // ascending sphere order, so images and g-buffers are bit-identical; only the executed-tests and
  // row-cost counters change.
  static constexpr bool SORT = false;
  // The pool's primary-ray cull masks loaded from FrameParams::cull (cull_fill_kernel wrote them
  // with the pool start's own code) instead of computed: pool_cone_f and cone_misses_f are not
  // compiled in.  All-sphere scenes only (planes would need a second table for pmask).
  static constexpr bool CULLC = false;
  // With SORT and CULLC: the sort keyed on the pool's cached sort frame (FrameParams::cull_frames,
  // cull_fill_kernel) when the launch has one: hemi's 45-degree sector around the surface normal
  // at the pool's centre ray instead of hemi's world octant.  The same bit-identical results.
  static constexpr bool NSORT = false;
  static constexpr int ABL = 0;        // diagnostics (A/B tools library): timing ablations, section clocks, event counts
};
// What the production launcher varies, as bits of AoProd's FLAGS / AoChoice::flags
enum : unsigned {
  AO_PL = 1,     // AoConfig::PL
  AO_CLON = 2,   // AoConfig::CLON
  AO_SORT = 4,   // AoConfig::SORT
  AO_WIDE = 8,   // above kTailMaxObj spheres: AoConfig::PTW (else the sphere table fits the LDS rows)
  AO_CNT = 16,   // AoConfig::CNT
  AO_MF = 32,    // AoConfig::MF
  AO_CULLC = 64, // AoConfig::CULLC
  AO_RC = 128,   // AoConfig::RC (with AO_PL)
};
// The forms that key the sort on the pool's frame: sorted and cached, not the counter forms (their
// work counters stay those of the uncached launch, whose key is the octant), never with planes.
constexpr bool ao_sorts_by_frame(unsigned flags) {
  return (flags & (AO_SORT | AO_CULLC | AO_CNT | AO_PL)) == (AO_SORT | AO_CULLC);
}
// A production configuration: split tail rounds, the batched first bounce and its pre-test always.
template <int SPPC_, int DC_, unsigned FLAGS>
struct AoProd : AoConfig {
  static constexpr int SPPC = SPPC_, DC = DC_;
  static constexpr bool RC = FLAGS & AO_RC;
  static constexpr bool PL = FLAGS & AO_PL, CLON = FLAGS & AO_CLON, SORT = FLAGS & AO_SORT, PTW = FLAGS & AO_WIDE,
                        CNT = FLAGS & AO_CNT, MF = FLAGS & AO_MF, CULLC = FLAGS & AO_CULLC,
                        NSORT = ao_sorts_by_frame(FLAGS);
  static constexpr bool TAIL = true, B1 = true, PT = true;
};

// LDS layout of ao_batch_kernel<C>, in bytes.  Every offset is a compile-time constant when spp
// is (C::SPPC), so the kernel then holds no LDS addresses in scalar registers.
struct BatchLds {
  int prec, sres, pstop, pkind, perm, order, cmask, rls, geol, total;
};
__host__ __device__ constexpr BatchLds batch_lds_of(int spp, int ntail, bool rls_lds, bool sort) {
  const int TP = kPool / spp > 0 ? kPool / spp : 1, NS = TP * spp;
  BatchLds L{};
  L.prec = 0;                                   // [TP] float4: first-segment (normal, t) of sample 0
  L.sres = 16 * TP;                             // [3][NS] float: per-sample r, g, b (channel-major)
  L.pstop = L.sres + 12 * NS;                   // [TP] int: max (aa << 16 | stop) of the stop writes
  L.pkind = L.pstop + 4 * TP;                   // [TP] int
  L.perm = L.pkind + 4 * ((TP + 1) & ~1);       // [64] int: live rank -> lane of the prepared batch
  L.order = L.perm + 256;                       // [kPool] u8: batch slot -> item (SORT only)
  L.cmask = (L.order + (sort ? kPool : 0) + 7) & ~7;  // [32] u64: primary cull mask (nobj <= 2048)
  L.rls = (L.cmask + 8 * 32 + 15) & ~15;        // [2 spp] float4: rand_buffer (rls_lds)
  L.geol = L.rls + (rls_lds ? 32 * spp : 0);    // [ntail] float4: sphere table (split tail rounds) / pre-test rows
  L.total = L.geol + 16 * ntail;
  return L;
}
// configuration C's layout: no rand_buffer copy with PTW, order[] with SORT
template <class C>
__host__ __device__ constexpr BatchLds batch_lds(int spp, int ntail) {
  return batch_lds_of(spp, ntail, !C::PTW, C::SORT);
}

// The SORT pre-pass keyed on a pool's sort frame (e1, e2): a sample's three bits are a < 0 (bit 0),
// b < 0 (bit 1) and |a| < |b| (bit 2) of a = dot(hemi, e1), b = dot(hemi, e2), i.e. the 45-degree
// sector of hemi's azimuth around the normal.  sector_bits: the bits of a point; sector_code(s):
// the bits of sector s, [45 s, 45 s + 45) degrees from e1 towards e2.  The sort's bin s holds
// sector s, so neighbouring bins (and the last and the first) are neighbouring sectors.
constexpr int sector_bits(float a, float b) {
  return (a < 0.0f ? 1 : 0) | (b < 0.0f ? 2 : 0) | ((a < 0.0f ? -a : a) < (b < 0.0f ? -b : b) ? 4 : 0);
}
__host__ __device__ constexpr int sector_code(int s) { return (int)(0x26731540u >> (4 * s)) & 7; }
constexpr bool sector_code_ok() {
  // a point inside each sector, counter-clockwise from e1
  constexpr float pa[8] = {2, 1, -1, -2, -2, -1, 1, 2}, pb[8] = {1, 2, 2, 1, -1, -2, -2, -1};
  unsigned seen = 0;
  for (int s = 0; s < 8; ++s) {
    if (sector_code(s) != sector_bits(pa[s], pb[s])) return false;
    const int d = sector_code(s) ^ sector_code((s + 1) & 7);  // neighbours differ in one compare
    if (d != 1 && d != 2 && d != 4) return false;
    seen |= 1u << sector_code(s);
  }
  return seen == 0xffu;  // a permutation of the 8 codes
}
static_assert(sector_code_ok(), "sector_code: the 8 sectors in circular order");

// The pool list in front of a cull table's sort frames (rt_kernels.h ao_pool_list_bytes), addressed
// from the mask table's pointer as the frames are: the rows upwards from the list's first byte, the
// sky list downwards from the rows' end, where the chunk counts start.
__device__ __forceinline__ const int4* pool_list_rows(const void* table, unsigned pools) {
  return (const int4*)((const char*)table - ao_cull_frame_bytes(pools) - ao_pool_list_bytes(pools));
}
__device__ __forceinline__ const unsigned* pool_list_sky_end(const void* table, unsigned pools) {
  return (const unsigned*)(pool_list_rows(table, pools) + pools);
}

// A sky block of a pool-list launch (FrameParams::cull_frames == 2): sky pools [first, first + 64)
// of the list, one pixel per lane and step.  What the pool's own sky exit stores (below), pixel for
// pixel: the same float sequence for the colour, through the same stores.  No LDS, no barrier.
// npix < 2^31 (the cull cache builds no list above), so a pixel's index is a 32-bit number.
template <int SPPC>
__device__ __forceinline__ void ao_sky_block(const FrameParams& P, const unsigned* __restrict__ sky_end, unsigned first,
                                             unsigned nsky, unsigned npix) {
  const int spp = SPPC ? SPPC : P.spp;
  const unsigned TP = kPool / spp > 0 ? kPool / spp : 1, W = (unsigned)P.W;
  const float fa = (float)spp;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f;
  for (int k = 0; k < spp; ++k) {
    sr = sr + 1.0f * P.bg.x; sg = sg + 1.0f * P.bg.y; sb = sb + 1.0f * P.bg.z;
  }
  const float4 col = gamma_out(sr / fa, sg / fa, sb / fa);
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (unsigned e = threadIdx.x; e < 64u * TP; e += 64) {
    const unsigned q = e / TP, j = first + q;
    if (j >= nsky) break;  // (j grows with e: the lanes past the list's end are done)
    const unsigned pix = sky_end[-1 - (long long)j] * TP + (e - q * TP);
    if (pix >= npix) continue;  // the frame's last pool may be partial
    const unsigned yr = pix / W;
    const int x = (int)(pix - yr * W), y = P.trace_row0 + (int)yr;
    const size_t off = (size_t)(y - P.band_row0) * W + x;
    nrm_store(P.nrm, dep_plane(P), off, z);
    dep_store(P.dep, dep_plane(P), off, z);
    store_color(P, P.out_pix, P.image, x, y, col);
  }
}

// geo: the sphere table (P.sph).  The bounce-ray cluster cull of the later bounce rounds runs
// whenever the launch has clusters (P.ncl > 0); without them the rounds test every sphere.
// cullt: the pools' cull masks (P.cull), read by CULLC only; an argument of its own, read-only and
// non-aliased like geo, so that its wave-uniform loads are scalar loads.
template <class C>
__global__ __launch_bounds__(64, kAoMinWaves) void ao_batch_kernel(FrameParams P, const float4* __restrict__ geo,
                                                                   const unsigned long long* __restrict__ cullt) {
  constexpr int SPPC = C::SPPC, DC = C::DC, ABL = C::ABL;
  constexpr bool PL = C::PL, CLON = C::CLON, CNT = C::CNT, MF = C::MF, LAZY = C::LAZY, TAIL = C::TAIL, B1 = C::B1,
                 PT = C::PT, PTW = C::PTW, SORT = C::SORT, CULLC = C::CULLC;
  static_assert(!CULLC || !PL, "the cull table holds the spheres' masks only");
  constexpr bool RC = C::RC;
  static_assert(!RC || PL, "rectangles are entries of the plane table");
  constexpr bool NSORT = C::NSORT;
  static_assert(!NSORT || (CULLC && SORT), "the sort frames come with the cull table");
  __builtin_amdgcn_s_setprio(1);  // the pool's start at issue priority 1, back to 0 after the primary cull
  // CNT = false: the work counters compiled out (timed launches pass none): fewer live scalars
  unsigned long long* const cnts = CNT ? P.counters : nullptr;
  unsigned long long* const rowc = CNT ? P.row_counters : nullptr;
  extern __shared__ float4 lds[];
  const int spp = SPPC ? SPPC : P.spp, W = P.W, D = DC ? DC : P.D, nobj = P.nobj;
  // CLON: launched only with clusters (P.ncl > 0), so the rounds' plain full-scan path is not compiled
  const bool use_cl = CLON || P.ncl > 0;
  // this frame's buffers (the launch's frame unless MF)
  const int fj = MF ? (int)blockIdx.y : 0;
  const int fslot = MF ? (P.mf_slot0 + fj) % P.F : 0;
  float4* const f_nrm = MF ? (float4*)P.hist_nrm[fslot] : P.nrm;
  float4* const f_dep = MF ? (float4*)P.hist_dep[fslot] : P.dep;
  const float4* const f_nrm_prev = MF ? f_nrm : P.nrm_prev;  // sequential frames: the slot itself
  const float4* const f_dep_prev = MF ? f_dep : P.dep_prev;
  float4* const f_out = MF ? (float4*)P.hist_pix[fslot] : P.out_pix;
  float4* const f_img = MF ? (fj == P.mf_n - 1 ? P.image : nullptr) : P.image;
  const float4* const f_rb = MF ? P.mf_rb + (size_t)fj * 2 * spp : P.rb;
  const int TP = kPool / spp > 0 ? kPool / spp : 1;
  const int lane = threadIdx.x;
  const int NS = TP * spp;
  // A pool-list launch (FrameParams::cull_frames == 2; the single-frame forms that take frames):
  // the blocks behind the non-sky pools' store the list's sky pools, before any LDS is touched.
  constexpr bool LIST = NSORT && !MF;
  bool listed = false;  // wave-uniform
  unsigned list_pools = 0;
  if constexpr (LIST) {
    listed = P.cull_frames == 2;
    if (listed) {
      const unsigned npx = (unsigned)P.trace_rows * (unsigned)W, nns = (unsigned)P.pool_rot;
      list_pools = (npx + (unsigned)TP - 1) / (unsigned)TP;
      if (blockIdx.x >= nns) {
        __builtin_amdgcn_s_setprio(0);
        ao_sky_block<SPPC>(P, pool_list_sky_end(cullt, list_pools), (blockIdx.x - nns) * 64, list_pools - nns, npx);
        return;
      }
    }
  }
  // PTW (scenes above kTailMaxObj spheres): the first bounce's pre-test rows one 64-sphere word at a
  // time in LDS, the split tail rounds on the global table, and rand_buffer read from global memory
  // (its LDS copy would not leave room for the rows at 7 waves per SIMD with spp 64)
  static_assert(!SORT || (LAZY && kPool % 64 == 0 && kPool <= 256), "SORT: hemi is read back from LDS; items are bytes");
  const BatchLds LO = batch_lds<C>(spp, 0);
  char* lbase = (char*)lds;
  float4* prec = (float4*)(lbase + LO.prec);
  float* sres = (float*)(lbase + LO.sres);
  int* pstop = (int*)(lbase + LO.pstop);
  int* pkind = (int*)(lbase + LO.pkind);
  int* perm = (int*)(lbase + LO.perm);
  unsigned char* order = (unsigned char*)(lbase + LO.order);  // SORT
  unsigned long long* cmask = (unsigned long long*)(lbase + LO.cmask);
  float4* rls = (float4*)(lbase + LO.rls);
  if (!PTW)
    for (int k = lane; k < 2 * spp; k += 64) rls[k] = f_rb[k];
  for (int k = lane; k < TP; k += 64) pstop[k] = -1;
  // TAIL: the sphere table in LDS (per-lane sphere indices in the split tail rounds)
  float4* geol = (float4*)(lbase + LO.geol);  // [nobj] when TAIL && nobj <= kTailMaxObj
  // split tail rounds: the sphere table in LDS up to kTailMaxObj spheres; above (TAIL instantiations
  // launched without the LDS table), per-lane reads of the global table (L1/L2-resident)
  constexpr bool tail_lds = TAIL && PT && !PTW;  // the LDS-table configurations (<= kTailMaxObj spheres) have PT
  const bool tail_ok = TAIL;
  const float4* const tgeo = tail_lds ? geol : geo;
  // PT: the batched first bounce keeps its per-ray pre-test table in the same LDS rows, so the
  // sphere table is (re)staged only when a split tail round needs it
  const bool pt_ok = PT && B1 && (tail_lds || PTW);
  bool geol_valid = false;  // wave-uniform
  if (tail_lds && !pt_ok) {
    for (int k = lane; k < nobj; k += 64) geol[k] = geo[k];
    geol_valid = true;
  }
  // the cluster table and masks (rt_kernels.h layout: shapes + 7S, i.e. geo + 3S) read through the
  // read-only, non-aliased sphere-table pointer: their wave-uniform loads in the bounce rounds are
  // then scalar loads (through FrameParams they were vector loads, one memory round trip each)
  const float4* const clus = geo + (size_t)3 * P.S;
  const unsigned long long* const clm = (const unsigned long long*)(geo + (size_t)3 * P.S + kMaxClusters);
  // col[ind] / aux[ind] (rt_device.h scene tables) addressed from the sphere table (geo = shapes + 4S, launch_program) with a
  // per-lane offset the compiler cannot fold into a hoisted pointer: the two extra 64-bit base
  // pointers were the most reloaded of the kernel's scalar spills (a v_readlane pair each, per shade)
  auto col_at = [&](int ind) -> float4 {
    int o = ind - P.S;
    asm("" : "+v"(o));
    return geo[o - P.S];
  };
  auto aux_at = [&](int ind) -> float4 {
    int o = ind - P.S;
    asm("" : "+v"(o));
    return geo[o];
  };

  const long long npix = (long long)P.trace_rows * W;
  // pool of this workgroup
  unsigned pb = blockIdx.x;
  // XCD balance: workgroups are dealt round-robin to the 8 XCDs (b mod 8), so in row order an XCD
  // would take the same pool columns in every row (the same 16-px column stripes of the image);
  // rotating row r's pools by r (groups of pool_rot = pools per row) moves each XCD's columns by
  // one pool per row, so over 8 rows every XCD samples every column residue (a bijection on the
  // full groups; the last, partial group keeps its order).  Config (d) AO launch: -3%.
  // A pool-list launch reads pb and the pool's (xf, yf, np) below from the block's row instead (one
  // scalar load: a wave-uniform address); the rotation and the divisions are not executed.
  int4 row = make_int4(0, 0, 0, 0);
  if (LIST && listed) {
    row = pool_list_rows(cullt, list_pools)[blockIdx.x];
    pb = (unsigned)row.x;
  } else if (P.pool_rot > 0) {
    const unsigned Q = (unsigned)P.pool_rot, r = pb / Q;
    if ((r + 1) * Q <= gridDim.x) {
      unsigned c = pb - r * Q + r % Q;
      c = c >= Q ? c - Q : c;
      pb = r * Q + c;
    }
  }
  const long long p0 = (long long)pb * TP;  // (not read by a pool-list launch)
  const int np = LIST && listed ? row.w : (int)(npix - p0 < TP ? npix - p0 : TP);
  const int total = np * spp;

  // ABL == 3: per-section wave clock (s_memtime) into the counters, timing ablation only
  unsigned long long tsec[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // 5..7: bounce rounds, sum ncull, prepares
  // ABL == 6: the same, with slots 5..7 timing the batched first bounce's cone + cull, survivor
  // loop and shading; ABL == 7: event counts of the first bounce and the bounce rounds instead
  // ABL == 8: the ABL == 3 sections with the later bounce rounds split: split tail rounds in slot
  // 5, full rounds in slot 3; slots 6 / 7 count full / tail rounds
  constexpr bool kLaps = ABL == 3 || ABL == 6 || ABL == 8;
  unsigned long long tmark = kLaps ? __builtin_amdgcn_s_memtime() : 0;
  auto lap = [&](int k) {
    if (kLaps) {
      unsigned long long now = __builtin_amdgcn_s_memtime();
      tsec[k] += now - tmark;
      tmark = now;
    }
  };
  // ---- frustum cull of the primary rays -------------------------------------------------
  // once per pool (scalar)
  const int yf = LIST && listed ? row.z : P.trace_row0 + (int)(p0 / W), xf = LIST && listed ? row.y : (int)(p0 % W);
  // pixel lp of the pool: (xf + lp, yf), wrapped into the next row(s) when it passes W
  auto pool_xy = [&](int lp, int& x, int& y) {
    int xi = xf + lp;
    y = yf;
    if (xi >= W) {  // only pools that straddle a row end (none when TP divides W)
      int q = (int)((unsigned)xi / (unsigned)W);
      y += q;
      xi -= q * W;
    }
    x = xi;
  };
  const int yl = P.trace_row0 + (int)((p0 + np - 1) / W), xl = (int)((p0 + np - 1) % W);
  int ncull = 0;
  const int nwords = (nobj + 63) >> 6;
  unsigned long long pmask = 0;  // PL: planes k < 64 the pool's camera rays may hit (wave-uniform)
  if constexpr (CULLC) {
    // the masks of pool pb as cull_fill_kernel computed them (wave-uniform address: scalar loads)
    const unsigned long long* const ct = cullt + (size_t)pb * (unsigned)nwords;
#pragma nounroll
    for (int w = 0; w < nwords; ++w) {
      const unsigned long long m = ct[w];
      ncull += __popcll(m);
      if (lane == 0) cmask[w] = m;
    }
  } else {
    const ConeF cone = pool_cone_f(P, yf == yl ? xf : 0, yf == yl ? xl : W - 1, yf, yl);
    for (int w = 0; w < nwords; ++w) {
      int i = (w << 6) + lane;
      bool keep = i < nobj && !cone_misses_f(cone, geo[i], P.cx, P.cy, P.cz);
      if (PL) keep = keep && geo[i].x == geo[i].x;  // not a plane / other shape (NaN in the sphere table)
      unsigned long long m = __ballot(keep);
      ncull += __popcll(m);
      if (lane == 0) cmask[w] = m;
    }
    if (PL) {
      pmask = plane_cone_mask(P, cone, mk(P.cx, P.cy, P.cz));
      ncull += __popcll(pmask) + (P.nplanes > 64 ? P.nplanes - 64 : 0);
    }
  }
  __syncthreads();
  lap(0);
  __builtin_amdgcn_s_setprio(0);

  if (LAZY && ncull == 0) {
    // Empty frustum: every primary ray of the pool provably misses every sphere, so each
    // sample is "miss at the first segment": colour 1*background, depth.y = 0, zero g-buffer.
    // Same float sequence as the general path (sum of spp background values, then / spp).
    const float fa = (float)spp;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (int k = 0; k < spp; ++k) {
      sr = sr + 1.0f * P.bg.x; sg = sg + 1.0f * P.bg.y; sb = sb + 1.0f * P.bg.z;
    }
    const float4 col = gamma_out(sr / fa, sg / fa, sb / fa);
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int lp = lane; lp < np; lp += 64) {
      int x, y;
      pool_xy(lp, x, y);
      const size_t off = (size_t)(y - P.band_row0) * W + x;
      nrm_store(f_nrm, dep_plane(P), off, z);
      dep_store(f_dep, dep_plane(P), off, z);  // (0, 0, 0, 0) / AA
      store_color(P, f_out, f_img, x, y, col);
      if (rowc) atomicAdd(&rowc[y - P.band_row0], (unsigned long long)spp);  // ~free
    }
    if (cnts && lane == 0 && ABL < 3) {  // (ABL >= 3: the counters hold section clocks / events)
      unsigned long long* c = cnts + (blockIdx.x & (kCounterSlots - 1));
      atomicAdd(&c[0 * kCounterSlots], (unsigned long long)total);
      atomicAdd(&c[1 * kCounterSlots], (unsigned long long)total);
      atomicAdd(&c[3 * kCounterSlots], (unsigned long long)total * (unsigned long long)nobj);
      // the pool's cull is the scene loop of these segments: every sphere tested once for the whole
      // pool, one per lane, on nwords rounds of the wave (counted so when the masks were loaded too)
      atomicAdd(&c[4 * kCounterSlots], 64ull * (unsigned long long)nwords);
    }
    return;
  }

  const f3 cam = mk(P.cx, P.cy, P.cz);
  const float4* rbuf = PTW ? f_rb : rls;
  // live path of this lane
  bool has = false;
  int item = 0, depth = 0;
  f3 pos = cam, dir = cam, hemi = cam;
  float rr = 1.0f, rg = 1.0f, rb = 1.0f;
  // prepared batch slot of this lane
  int bitem = 0;
  f3 bpos = cam, bdir = cam, bhemi = cam;
  float br = 1.0f, bg = 1.0f, bb = 1.0f;
  int next = 0, cursor = 0, nlive = 0, bdepth = D - 1;  // wave-uniform
  int b1cost = nobj;  // spheres the latest batched first bounce tested (row cost profile)
  unsigned nseg = 0;
  unsigned long long exec_tests = 0;

  const float inv_spp = P.inv_spp;
  // it / spp for pool items (< 2^16): exact via the float reciprocal (error << 0.5/spp)
  auto div_spp = [&](int it) { return SPPC ? (int)((unsigned)it / (unsigned)SPPC) : (int)(((float)it + 0.5f) * inv_spp); };
  // row cost profile (strip balancing), in sphere-test units: setup + culled primary + bounces
  auto finish = [&](int it, float r, float g, float b, float stopv, int segs) {
    sres[it] = r;
    sres[NS + it] = g;
    sres[2 * NS + it] = b;
    if (stopv >= 0.0f) {  // depth_buffer.y: the last writer in sample order wins
      const int lq = div_spp(it);
      atomicMax(&pstop[lq], ((it - lq * spp) << 16) | (int)stopv);
    }
    if (rowc) {
      int x, y;
      pool_xy(div_spp(it), x, y);
      atomicAdd(&rowc[y - P.band_row0],
                (unsigned long long)(kSetupCost + ncull + (segs >= 2 ? b1cost + (segs - 2) * nobj : 0)));
    }
  };

  // hit shading shared by primary and bounce segments; returns true when the path goes on
  // (written with one exit: the attenuation product, the kind store and finish() each appear
  // once, and the diffuse and mirror directions share their final normalize, so lanes that
  // take different cases do not run duplicated code)
  auto shade = [&](int ind, float t, f3& ps, f3& dr, f3 hm, float& r, float& g, float& b, int dpt, int it,
                   bool first) -> bool {
    const int lp = div_spp(it), aa = it - lp * spp;
    // a miss (ind == -1) reads the background: the host stores it as the colour table's row -1
    float4 att = col_at(ind);
    int kind = PRIM_MISS;
    bool go = false;
    if (ind != -1) {
      const float4 ax = aux_at(ind);
      // all-sphere scenes: the hit sphere's centre requested with its colour and flags, one memory
      // round trip (pinned here: the compiler would sink the load behind the emissive test)
      float4 gc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (!PL) {
        gc = geo[ind];
        asm volatile("" ::"v"(gc.x), "v"(gc.y), "v"(gc.z));
      }
      if (ax.x > 0.9f) {
        kind = PRIM_EMISSIVE;
      } else {
        kind = PRIM_HIT;
        f3 curr = cam + t * dr;  // sic: camera origin (ao_compute.glsl:210)
        f3 nn;
        if (PL) {  // ao_compute.glsl:211-218: the stored normal of a plane
          const float4 gi = P.shapes[ind];
          const int id = __float_as_int(P.shapes[P.S + ind].w);  // (RC: a rectangle's stored normal, as a plane's)
          nn = (RC ? id != SHAPE_SPHERE : id == SHAPE_PLANE) ? xyz(gi) : normalize(curr - xyz(gi));
        } else {
          nn = normalize(curr - xyz(gc));
        }
        if (aa == 0 && first) prec[lp] = make_float4(nn.x, nn.y, nn.z, t);
        if (ABL == 9) {  // instruction-budget ablation: the hit shading's arithmetic twice
          float z;
          asm volatile("v_mov_b32 %0, 0" : "=v"(z));
          const f3 c2 = cam + (t + z) * dr;
          const f3 n2 = normalize(c2 - (PL ? xyz(P.shapes[ind]) : xyz(gc)));
          const float d2 = dot(dr, n2);
          const f3 R2 = normalize(mk(dr.x - 2.0f * (d2 * n2.x), dr.y - 2.0f * (d2 * n2.y), dr.z - 2.0f * (d2 * n2.z)));
          const f3 X2 = normalize(ax.y > 0.999f ? hm + n2 : R2 + ax.y * hm);
          if (__float_as_uint(X2.x + X2.y + X2.z) == 0x7fc00001u) t = X2.x;
        }
        ps = curr;
        const float reflect = ax.y;
        f3 X;
        if (reflect > 0.999f) {
          X = hm + nn;
        } else {
          float dn = dot(dr, nn);
          f3 R = normalize(mk(dr.x - 2.0f * (dn * nn.x), dr.y - 2.0f * (dn * nn.y), dr.z - 2.0f * (dn * nn.z)));
          X = R + reflect * hm;
        }
        dr = normalize(X);
        go = dpt - 1 != 0;  // RECURSION_DEPTH non-emissive hits end without a stop write
      }
    }
    r = r * att.x; g = g * att.y; b = b * att.z;
    if (aa == 0 && first) pkind[lp] = kind;
    if (!go) finish(it, r, g, b, kind == PRIM_HIT ? -1.0f : (float)(D - dpt), kind == PRIM_HIT ? D : D - dpt + 1);
    return go;
  };

  // Prepare the next 64 samples with the whole wave.
  auto prepare = [&]() {
    bitem = next + lane;
    bool live = false;
    if (ABL == 3) { tsec[6] += (unsigned long long)ncull; tsec[7] += 1; }
    exec_tests += (unsigned long long)ncull;
    if (bitem < total) {
      if (SORT) bitem = order[bitem];  // the pool's samples in bounce-direction order
      const int lp = div_spp(bitem), aa = bitem - lp * spp;
      int x, y;
      pool_xy(lp, x, y);
      const float px = (float)x, py = (float)y;
      float hp, vp;
      {  // ao_compute.glsl:310-323; sample 0 is unjittered: px + 0 == px, so one path for
        // every lane (no divergent branch in the batch)
        float4 f = rbuf[2 * aa], s = rbuf[2 * aa + 1];
        float uw[2];
        grandom_n<2>({((s.x + px * f.z) - px) + f.x, s.z * px - (f.x * px) * f.z},
                     {((f.y + py * s.w) - py) + s.y, f.w * py - (s.y * py) * s.w}, uw);
        if (ABL == 4) {  // instruction-budget ablation: the jitter hashes twice
          float z, uw2[2];
          asm volatile("v_mov_b32 %0, 0" : "=v"(z));
          grandom_n<2>({((s.x + px * f.z) - px) + f.x + z, s.z * px - (f.x * px) * f.z + z},
                       {((f.y + py * s.w) - py) + s.y, f.w * py - (s.y * py) * s.w}, uw2);
          if (__float_as_uint(uw2[0]) == 0x7fc00001u && __float_as_uint(uw2[1]) == 0x7fc00001u) uw[0] = uw2[0];
        }
        float u = uw[0], w = uw[1];
        normalize2(u, w);
        const float jx = aa == 0 ? 0.0f : div_rn_by(u, 6.0f, kInv6) - 0.08333f;
        const float jy = aa == 0 ? 0.0f : div_rn_by(w, 6.0f, kInv6) - 0.08333f;
        hp = div_rn_by(px + jx, P.fW, P.inv_W);
        vp = div_rn_by(py + jy, P.fH, P.inv_H);
      }
      bdir = primary_dir(P, hp, vp);
      if (ABL == 10) {  // instruction-budget ablation: the primary setup after the hashes twice
        float z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        float u2 = hp + z, w2 = vp + z;
        normalize2(u2, w2);
        const float jx2 = aa == 0 ? 0.0f : div_rn_by(u2, 6.0f, kInv6) - 0.08333f;
        const float jy2 = aa == 0 ? 0.0f : div_rn_by(w2, 6.0f, kInv6) - 0.08333f;
        const f3 d2 = primary_dir(P, div_rn_by(px + jx2, P.fW, P.inv_W), div_rn_by(py + jy2, P.fH, P.inv_H));
        if (__float_as_uint(d2.x + d2.y + d2.z) == 0x7fc00001u) bdir.x = d2.y;
      }
      // get_pt_within_unit_sphere(aa), hoisted: it depends on aa and the pixel only, so it is
      // computed once per sample — after the primary hit when LAZY, for hits only (a non-emissive
      // hit uses it)
      auto hemisphere = [&]() {
        float4 f = rbuf[2 * aa], s = rbuf[2 * aa + 1];
        float abe[3];
        grandom_n<3>({f.x + px * s.z, f.z - px * s.z, s.x * px + s.z}, {f.y + py * s.w, f.w - py * s.w, s.y * py + s.w},
                     abe);
        if (ABL == 4) {  // instruction-budget ablation: the hemisphere hashes twice
          float z, abe2[3];
          asm volatile("v_mov_b32 %0, 0" : "=v"(z));
          grandom_n<3>({f.x + px * s.z + z, f.z - px * s.z + z, s.x * px + s.z + z},
                       {f.y + py * s.w, f.w - py * s.w, s.y * py + s.w}, abe2);
          if (__float_as_uint(abe2[0]) == 0x7fc00001u && __float_as_uint(abe2[2]) == 0x7fc00001u) abe[1] = abe2[1];
        }
        return normalize(mk(abe[0] * 2.0f - 1.0f, abe[1] * 2.0f - 1.0f, abe[2] * 2.0f - 1.0f));
      };
      if (!LAZY) bhemi = hemisphere();
      // the camera in VGPRs for the primary tests: with the uniform camera and the sphere both in
      // SGPRs, each of the three subtractions would need a copy first (one scalar operand per
      // vector instruction)
      f3 cv = cam;
      asm("" : "+v"(cv.x), "+v"(cv.y), "+v"(cv.z));
      bpos = cv;
      br = bg = bb = 1.0f;
      float t = -1.0f;
      int ind = -1;
      for (int w = 0; w < nwords; ++w) {
        unsigned long long m = cmask[w];
        m = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
            (unsigned)__builtin_amdgcn_readfirstlane((unsigned)m);
        const float4* const gw = geo + (w << 6);  // (unsigned row offset: see the bounce rounds)
        while (m) {
          const unsigned j = (unsigned)pop_lowest(m);
          const int i = (w << 6) + (int)j;
          sphere_candidate(bpos, bdir, gw[j], i, 0.0001f, t, ind);
          if (ABL == 2) {  // timing ablation: the culled primary tests twice
            float z;
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            float t2 = -1.0f;
            int i2 = -1;
            sphere_candidate(mk(bpos.x + z, bpos.y, bpos.z), bdir, geo[i], i, 0.0001f, t2, i2);
            if (i2 == 0x7fffffff) t = t2;
          }
        }
      }
      if (PL) plane_pass_masked<RC>(P, pmask, bpos, bdir, 0.0001f, t, ind);
      ++nseg;
      // (every hit, emissive or not: only non-emissive hits use it, but waiting for the hit's flags
      // first cost a memory round trip, and a wave with any non-emissive hit computes it anyway)
      // (SORT: computed by the pool's pre-pass and parked in the sample's sres slots, which finish() overwrites)
      if (LAZY && ind != -1) bhemi = SORT ? mk(sres[bitem], sres[NS + bitem], sres[2 * NS + bitem]) : hemisphere();
      live = shade(ind, t, bpos, bdir, bhemi, br, bg, bb, D, bitem, true);
    }
    bdepth = D - 1;
    b1cost = nobj;
    if (B1) {
      // The batch's live paths take their first bounce together, against the spheres their
      // bounce cone does not exclude (bounce_cone), in ascending index order as closest_hit.
      const unsigned long long lm1 = __ballot(live);
      if (lm1 != 0 && __popcll(lm1) >= P.b1_min) {
        lap(1);
        __builtin_amdgcn_s_setprio(1);  // the batched first bounce at issue priority 1, every other phase at 0
        const ConeB cb = bounce_cone(live, bpos, bdir, lm1);
        float t = -1.0f;
        int ind = -1;
        b1cost = 0;
        if (ABL == 12) {  // instruction-budget ablation: the first bounce's cone and cull twice
          float z;
          asm volatile("v_mov_b32 %0, 0" : "=v"(z));
          const ConeB c2 = bounce_cone(live, mk(bpos.x + z, bpos.y, bpos.z), bdir, lm1);
          unsigned long long acc = 0;
          for (int w = 0; w < nwords; ++w) {
            const int i = (w << 6) + lane_id_here();
            float4 pt;
            const bool k2 = i < nobj && bounce_cone_keep_pt(c2, geo[i], pt);
            acc ^= __ballot(k2 && pt.w != 7.0f);
          }
          if (acc == 0x123456789abcdefull) b1cost = 1;
        }
        // The exact tests of the survivors whose pre-test passes somewhere are
        // deferred and merged: survivors whose pass masks are disjoint share one exact-test
        // pass, each lane testing the one sphere it passed (ksel, read per lane); a survivor
        // whose mask meets the pending ones first runs them.  Every lane still meets its spheres
        // in ascending index order, so (t, ind) is the sequential scan's.
        // (Two pending spheres per lane, flushed when a lane would need a third: no better,
        // profiles/r05z4_*.)
        unsigned long long ru = 0;  // lanes with a pending sphere (wave-uniform)
        int ksel = 0;               // the pending sphere of each lane in ru
        // the pre-test's direction, NaN on the lanes that are not live (their pre-test then
        // fails, NaN >= K being false), so the ballot needs no live mask
        f3 tdir = bdir;
        if (!live) tdir = mk(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
        auto flush = [&]() {
          const float4 gs = geo[ksel];
          sphere_candidate_if(bpos, bdir, gs, ksel, 0.0001f, t, ind, ru);
          ru = 0;
        };
        for (int w = 0; w < nwords; ++w) {
          // the lane index re-read here (not the kernel-wide one): otherwise the compiler keeps
          // this loop's per-lane addresses live across the whole pool and spills them to scratch
          const int i = (w << 6) + lane_id_here();
          bool keep;
          if (pt_ok) {
            float4 pt;
            keep = i < nobj && bounce_cone_keep_pt(cb, geo[i], pt);
            if (i < nobj) geol[PTW ? i - (w << 6) : i] = pt;  // (PTW: this word's rows only)
          } else {
            keep = i < nobj && !bounce_cone_misses(cb, geo[i]);
          }
          if (PL) keep = keep && geo[i].x == geo[i].x;  // planes are tested after the spheres
          unsigned long long m = __ballot(keep);
          m = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
              (unsigned)__builtin_amdgcn_readfirstlane((unsigned)m);
          exec_tests += (unsigned long long)__popcll(m);
          b1cost += __popcll(m);
          if (ABL == 3) tsec[6] += (unsigned long long)__popcll(m) << 24;  // sections: first-bounce survivors
          if (pt_ok) {
            geol_valid = false;
            __syncthreads();  // the pre-test rows are written
            if (ABL == 6) lap(5);
            const float4* const qw = geol + (PTW ? 0 : (w << 6));  // this word's rows and spheres (fewer
            const float4* const gw = geo + (w << 6);   // scalar address operations per survivor)
            // the row's LDS address is formed by one vector instruction from the row base held in
            // a VGPR (the compiler builds the uniform address with two scalar instructions and
            // copies it to a VGPR), and the broadcast read waits at once, as the loop would
            int qbase;
            asm("v_mov_b32 %0, %1" : "=v"(qbase) : "s"((int)(size_t)((const char*)qw - lbase)));
            // (the loop on every lane, the live lanes picked by lm1 in the ballots, so the pending
            // mask stays a scalar value across the loop)
            {
              while (m) {
                const int j = pop_lowest(m), k = (w << 6) + j;
                // the row read in C from the VGPR row base: one v_lshl_add_u32 for the address, the
                // compiler's own wait (no inline-asm boundary, whose hazard padding cost an s_nop)
                const float4 q = *(const float4*)(lbase + (qbase + (j << 4)));
                const float4 g = gw[j];
                if (ABL == 7) {  // survivor iterations; with any pre-test pass; with any del >= 0 there
                  const bool pass = fmaf(bdir.z, q.z, fmaf(bdir.y, q.y, bdir.x * q.x)) >= q.w;
                  const f3 pmc = bpos - xyz(g);
                  const float bb = dot(bdir, pmc);
                  const float del = fmaf(g.w, g.w, fmaf(bb, bb, -dot(pmc, pmc)));
                  const unsigned long long pm = __ballot(pass), dm = __ballot(pass && del >= 0.0f);
                  tsec[0] += 1; tsec[1] += pm != 0; tsec[2] += dm != 0;
                  tsec[3] += (unsigned long long)__popcll(pm);
                }
                // the skip as a branch on the ballot (VCC), not an exec-mask save / restore per survivor
                const bool pass = fmaf(tdir.z, q.z, fmaf(tdir.y, q.y, tdir.x * q.x)) >= q.w;
                if (ABL == 5) {  // instruction-budget ablation: each survivor iteration twice
                  float z, t2 = t;
                  int i2 = ind;
                  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                  const bool pass2 = fmaf(bdir.z + z, q.z, fmaf(bdir.y, q.y, bdir.x * q.x)) >= q.w;
                  const unsigned long long pm2 = __builtin_amdgcn_ballot_w64(pass2);
                  if (pm2 != 0) sphere_candidate_if(mk(bpos.x + z, bpos.y, bpos.z), bdir, g, k, 0.0001f, t2, i2, pm2);
                  if (i2 == 0x7fffffff) t = t2;
                }
                const unsigned long long pm = __builtin_amdgcn_ballot_w64(pass);
                if (pm != 0) {
                  if (pm & ru) flush();
                  ru |= pm;
                  int kv = k;
                  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(ksel) : "v"(ksel), "v"(kv), "s"(pm));
                }
              }
            }
            if (ABL == 6) lap(6);
          } else if (live) {
            while (m) {
              const int k = (w << 6) + __builtin_ctzll(m);
              m &= m - 1;
              sphere_candidate(bpos, bdir, geo[k], k, 0.0001f, t, ind);
            }
          }
        }
        if (ru != 0) flush();
        __builtin_amdgcn_s_setprio(0);
        if (ABL == 7) { tsec[4] += 1; tsec[5] += (unsigned long long)__popcll(lm1); }
        if (live) {
          if (PL) plane_pass<RC>(P, bpos, bdir, 0.0001f, t, ind);
          ++nseg;
          live = shade(ind, t, bpos, bdir, bhemi, br, bg, bb, D - 1, bitem, false);
        }
        if (ABL == 6) lap(7);
        bdepth = D - 2;
        lap(4);  // sections: the batched first bounce (shares slot 4 with combine + stores)
      }
    }
    unsigned long long lm = __ballot(live);
    if (live) perm[__builtin_amdgcn_mbcnt_hi((unsigned)(lm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lm, 0u))] = lane;
    nlive = __popcll(lm);
    cursor = 0;
    next = next + 64 < total ? next + 64 : total;
    __syncthreads();  // perm[] visible to the whole wave
  };

  if (SORT) {
    // ---- SORT pre-pass: hemi of every sample into its sres slots, order[] by hemi's octant ---
    // Counting sort over the cells (octant, chunk of 64 items), one cell per lane.  A lane's rank
    // among the chunk's lanes of its octant is a masked popcount of the chunk's three sign ballots;
    // the cell counts are scanned octant by octant (Gray-code order) and chunk by chunk inside an
    // octant, so the order is the same from run to run (items ascending inside an octant).
    // perm[] holds the cell table: it is free until the first prepare().
    constexpr int NC = kPool / 64, NF = 3;
    static_assert(NC * (1 << NF) <= 64, "one cell per lane");
    // NSORT, launched with the pools' sort frames (P.cull_frames): the three bits are those of
    // hemi's 45-degree sector around the pool's cached surface normal, a = dot(hemi, e1) < 0,
    // b = dot(hemi, e2) < 0, |a| < |b| (NaN and -0 by the compares' results: any bin is valid), and
    // the bins follow the sectors round the circle (sector_code).  (e1, e2): two scalar loads of
    // the pool's row in front of the mask table, through the table's own argument.
    bool framed = false;  // wave-uniform
    f3 fe1 = mk(0.0f, 0.0f, 0.0f), fe2 = fe1;
    if constexpr (NSORT) {
      framed = P.cull_frames != 0;
      if (framed) {
        const float4* const fr = (const float4*)cullt - 2 * ((size_t)pb + 1);
        fe1 = xyz(fr[0]);
        fe2 = xyz(fr[1]);
      }
    }
    const int ln = lane_id_here();
    perm[ln] = 0;
    __syncthreads();
    int key[NC];  // per chunk: rank in the cell | cell << 8
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      key[c] = 0;
      if (c * 64 < total) {  // wave-uniform
        const int it = c * 64 + ln;
        f3 h = mk(0.0f, 0.0f, 0.0f);  // (the lanes past total: octant 0, masked out below)
        if (it < total) {
          const int lp = div_spp(it), aa = it - lp * spp;
          int x, y;
          pool_xy(lp, x, y);
          const float px = (float)x, py = (float)y;
          // get_pt_within_unit_sphere(aa): prepare()'s hemisphere(), the same operations in the same order
          const float4 f = rbuf[2 * aa], s = rbuf[2 * aa + 1];
          float abe[3];
          grandom_n<3>({f.x + px * s.z, f.z - px * s.z, s.x * px + s.z}, {f.y + py * s.w, f.w - py * s.w, s.y * py + s.w},
                       abe);
          h = normalize(mk(abe[0] * 2.0f - 1.0f, abe[1] * 2.0f - 1.0f, abe[2] * 2.0f - 1.0f));
          sres[it] = h.x;
          sres[NS + it] = h.y;
          sres[2 * NS + it] = h.z;
        }
        // the chunk's lanes in this lane's octant (valid items only: the lanes past total are the
        // chunk's highest, so they precede no valid lane, but they would count in octant 0's cell)
        const int nv = total - c * 64;
        const unsigned long long mv = nv >= 64 ? ~0ull : (1ull << nv) - 1;
        unsigned own_lo = (unsigned)mv, own_hi = (unsigned)(mv >> 32);
        unsigned oct = 0;  // bit k = sign bit of component k (as the ballots: -0 and NaN by their sign bit)
        const float hc[NF] = {h.x, h.y, h.z};
        if (NSORT && framed) {
          const float a = dot(h, fe1), b = dot(h, fe2);
          const bool sb[NF] = {a < 0.0f, b < 0.0f, fabsf(a) < fabsf(b)};
#pragma unroll
          for (int k = NF - 1; k >= 0; --k) {
            const unsigned long long m = __ballot(sb[k]);
            const unsigned sgn = sb[k] ? ~0u : 0u;
            own_lo &= ~((unsigned)m ^ sgn);
            own_hi &= ~((unsigned)(m >> 32) ^ sgn);
            oct = oct << 1 | (unsigned)sb[k];
          }
        } else {
#pragma unroll
          for (int k = NF - 1; k >= 0; --k) {
            const int bits = __float_as_int(hc[k]);
            const unsigned long long m = __ballot(bits < 0);
            const unsigned sgn = (unsigned)(bits >> 31);
            own_lo &= ~((unsigned)m ^ sgn);
            own_hi &= ~((unsigned)(m >> 32) ^ sgn);
            oct = oct << 1 | (unsigned)bits >> 31;
          }
        }
        const int cell = (int)oct * NC + c;
        const int r = (int)__builtin_amdgcn_mbcnt_hi(own_hi, __builtin_amdgcn_mbcnt_lo(own_lo, 0u));
        if (it < total) perm[cell] = __popc(own_lo) + __popc(own_hi);  // (the same value from every lane of the cell)
        key[c] = r | cell << 8;
      }
    }
    __syncthreads();
    {  // lane = cell (bin ln / NC, chunk ln % NC) in sorted order: exclusive scan of the counts
      const int bin = ln / NC, c = ln % NC;
      const bool in = ln < NC * (1 << NF);
      // bin b holds octant b ^ (b >> 1): Gray code, neighbouring bins' octants differ in one sign;
      // framed: sector b's bits, the sectors in their order round the normal
      int cell = in ? (bin ^ (bin >> 1)) * NC + c : 0;
      if constexpr (NSORT) {
        if (framed) cell = in ? sector_code(bin & 7) * NC + c : 0;
      }
      const int n = in ? perm[cell] : 0;
      // inclusive scan on the DPP path: row_shr 1, 2, 4, 8 (zero fill) inside the rows of 16, then
      // row_bcast:15 into rows 1, 3 and row_bcast:31 into rows 2, 3
      int acc = n;
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x111, 0xf, 0xf, false);
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x112, 0xf, 0xf, false);
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x114, 0xf, 0xf, false);
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x118, 0xf, 0xf, false);
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x142, 0xa, 0xf, false);
      acc += __builtin_amdgcn_update_dpp(0, acc, 0x143, 0xc, 0xf, false);
      __syncthreads();  // every count is read
      if (in) perm[cell] = acc - n;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int it = c * 64 + ln;
      // slot < total: the cells partition the valid items, and a cell's base + its count <= total
      if (it < total) order[perm[key[c] >> 8] + (key[c] & 255)] = (unsigned char)it;
    }
    __syncthreads();  // order[] and the parked hemi visible to the wave
  }

  for (;;) {
    // ---- hand prepared live states to idle lanes; prepare more when the batch is used up --
    for (;;) {
      unsigned long long need = __ballot(!has);
      if (need == 0) break;
      if (cursor >= nlive) {
        if (next >= total) break;
        lap(2);
        prepare();
        lap(1);
        continue;
      }
      int r = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
      int take = __popcll(need) < nlive - cursor ? __popcll(need) : nlive - cursor;
      bool get = !has && r < take;
      int src = get ? perm[cursor + r] : lane;
      // every lane executes the shuffles (ds_bpermute reads the source lane's register)
      float sx = __shfl(bpos.x, src), sy = __shfl(bpos.y, src), sz = __shfl(bpos.z, src);
      float dx = __shfl(bdir.x, src), dy = __shfl(bdir.y, src), dz = __shfl(bdir.z, src);
      float hx = __shfl(bhemi.x, src), hy = __shfl(bhemi.y, src), hz = __shfl(bhemi.z, src);
      float cr = __shfl(br, src), cg = __shfl(bg, src), cb = __shfl(bb, src);
      int ci = __shfl(bitem, src);
      if (ABL == 11) {  // instruction-budget ablation: the hand-out's 13 shuffles twice
        int zi;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zi));
        const int s2 = src + zi;
        float q = __shfl(bpos.x, s2) + __shfl(bpos.y, s2) + __shfl(bpos.z, s2) + __shfl(bdir.x, s2) + __shfl(bdir.y, s2) +
                  __shfl(bdir.z, s2) + __shfl(bhemi.x, s2) + __shfl(bhemi.y, s2) + __shfl(bhemi.z, s2) + __shfl(br, s2) +
                  __shfl(bg, s2) + __shfl(bb, s2) + (float)__shfl(bitem, s2);
        if (__float_as_uint(q) == 0x7fc00001u) cr = q;
      }
      if (get) {
        pos = mk(sx, sy, sz);
        dir = mk(dx, dy, dz);
        hemi = mk(hx, hy, hz);
        rr = cr; rg = cg; rb = cb;
        item = ci;
        depth = bdepth;
        has = true;
      }
      cursor += take;
    }
    const unsigned long long hm = __ballot(has);
    if (hm == 0) break;
    lap(2);
    if (ABL == 3) tsec[5] += 1;
    // ---- split tail round: the pool has no fresh samples left and at most 32 paths are live.
    // Each live path gets a group of G = 64/2^ceil(log2 L) lanes; lane p of the group tests
    // spheres p, p+G, ... (ascending), and the group merges the partial results: minimum t,
    // lowest index on ties = exactly the sequential scan's result (ao_compute.glsl:183-194).
    const int L = __popcll(hm);
    if (tail_ok && next >= total && cursor >= nlive && L <= 32) {
      if (tail_lds && !geol_valid) {
        __syncthreads();
        for (int k = lane_id_here(); k < nobj; k += 64) geol[k] = geo[k];
        geol_valid = true;
      }
      int c = 0;
      while ((1 << c) < L) ++c;
      const int G = 64 >> c;  // the largest power of 2 with G * L <= 64
      const int rk = __builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u));
      if (has) perm[rk] = lane;
      __syncthreads();
      const int g = lane / G, pl = lane - g * G;
      const bool act = g < L;
      const int owner = act ? perm[g] : lane;
      const f3 o = mk(__shfl(pos.x, owner), __shfl(pos.y, owner), __shfl(pos.z, owner));
      const f3 d = mk(__shfl(dir.x, owner), __shfl(dir.y, owner), __shfl(dir.z, owner));
      float t = -1.0f;
      int ind = -1;
      if (use_cl && G <= kClusterTailMaxG) {
        // cluster cull over the round's L paths (cluster_may_hit): lane pl of group g tests
        // clusters pl, pl + G, ... for path g; the ballot folded over the groups gives the clusters
        // some path may hit.  Their spheres plus the always-tested ones, compacted in ascending
        // order into a byte list (LDS: the primary cull mask's words, dead once the pool's samples
        // are all prepared), are split over the group's lanes as before: the group merge below
        // returns the lexicographic minimum (t, index) over them = the full scan's result.
        unsigned long long kc = 0;
        for (int c0 = 0; c0 < P.ncl; c0 += G) {
          const int c = c0 + pl;
          const bool may = act && c < P.ncl && cluster_may_hit(o, d, clus[c]);
          unsigned long long b = __builtin_amdgcn_ballot_w64(may);
          for (int sh = 32; sh >= G; sh >>= 1) b |= b >> sh;
          kc |= (G == 64 ? b : (b & ((1ull << G) - 1))) << c0;
        }
        unsigned char* list = (unsigned char*)cmask;
        int cnt = 0;
        for (int w = 0; w < nwords; ++w) {
          unsigned long long m = clm[w];
          for (unsigned long long k2 = kc; k2;) m |= clm[(size_t)(1 + pop_lowest(k2)) * kClusterWords + w];
          const int ln = lane_id_here();
          if ((m >> ln) & 1ull)
            list[cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                (unsigned char)((w << 6) + ln);
          cnt += __popcll(m);
        }
        __syncthreads();  // the list is written (one wave per workgroup)
        exec_tests += (unsigned long long)((P.ncl + G - 1) / G + (cnt + G - 1) / G);
        if (act) {
          // the next list entry is requested before this one's test: one LDS round trip per
          // sphere (entry, then the sphere row) instead of two dependent ones
          int i = list[pl < cnt ? pl : 0];
          for (int k = pl; k < cnt; k += G) {
            const float4 g = tgeo[i];
            const int inext = list[k + G < cnt ? k + G : cnt - 1];  // (no exec-mask branch around it)
            sphere_candidate(o, d, g, i, 0.0001f, t, ind);
            i = inext;
          }
        }
      } else if (act) {
        for (int i = pl; i < nobj; i += G) sphere_candidate(o, d, tgeo[i], i, 0.0001f, t, ind);
      }
      for (int m = 1; m < G; m <<= 1) {
        const float tb = __shfl_xor(t, m);
        const int ib = __shfl_xor(ind, m);
        const bool take = ib >= 0 && (ind < 0 || tb < t || (tb == t && ib < ind));
        t = take ? tb : t;
        ind = take ? ib : ind;
      }
      float tt = __shfl(t, rk * G);
      int ii = __shfl(ind, rk * G);
      if (!(use_cl && G <= kClusterTailMaxG)) exec_tests += (unsigned long long)((nobj + G - 1) / G);
      if (has) {
        if (PL) plane_pass<RC>(P, pos, dir, 0.0001f, tt, ii);
        ++nseg;
        has = shade(ii, tt, pos, dir, hemi, rr, rg, rb, depth, item, false);
        depth -= 1;
      }
      if (ABL == 8) tsec[7] += 1;
      lap(ABL == 8 ? 5 : 3);
      continue;
    }
    // ---- one bounce segment for every live path, against every sphere ------------------
    exec_tests += (unsigned long long)(use_cl ? P.ncl : nobj);
    if (ABL == 7) {  // later bounce rounds: sphere iterations, and those with any live lane's del >= 0
      tsec[6] += (unsigned long long)nobj;
      for (int i = 0; i < nobj; ++i) {
        const float4 g = geo[i];
        const f3 pmc = pos - xyz(g);
        const float bb = dot(dir, pmc);
        const float del = fmaf(g.w, g.w, fmaf(bb, bb, -dot(pmc, pmc)));
        tsec[7] += __ballot(has && del >= 0.0f) != 0;
      }
    }
    if (use_cl) {
      // cluster cull: a cluster is skipped when no live lane's ray may hit it (cluster_may_hit);
      // the spheres of the kept clusters plus the always-tested ones are visited in ascending
      // index order, so (t, ind) is the full scan's (ao_compute.glsl:183-194)
      // Four clusters per step, their records requested together (one scalar-load round trip per
      // four; slots past ncl are still inside the table, the cluster masks follow the 64 slots,
      // and their bits are dropped below).  Every lane tests (a lane without a path only sets a
      // bit that the live mask drops), so the loop runs with the full exec mask.
      unsigned long long kc = 0;
      for (int c = 0; c < P.ncl; c += 4) {
        const float4 c0 = clus[c], c1 = clus[c + 1], c2 = clus[c + 2], c3 = clus[c + 3];
        // (the kept bits by scalar selects: the compiler's (b != 0) | ... << k went through VGPRs)
        const unsigned long long b0 = cluster_may_hit_mask(pos, dir, c0) & hm;
        const unsigned long long b1 = cluster_may_hit_mask(pos, dir, c1) & hm;
        const unsigned long long b2 = cluster_may_hit_mask(pos, dir, c2) & hm;
        const unsigned long long b3 = cluster_may_hit_mask(pos, dir, c3) & hm;
        // (bits 4..7 first and an opaque move before the shift: with bit 0 selected directly the
        // compiler builds it as a zero-extended bool through v_cndmask + v_readfirstlane)
        unsigned nib = (b0 ? 16u : 0u) | (b1 ? 32u : 0u) | (b2 ? 64u : 0u) | (b3 ? 128u : 0u);
        asm("" : "+s"(nib));
        kc |= (unsigned long long)(nib >> 4) << c;
      }
      // (bits of the slots past ncl need no mask: their member words are zero, rt_shim build_clusters)
      float t = -1.0f;
      int ind = -1;
      if (ABL == 13) {  // instruction-budget ablation: the cluster cull twice
        float z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        const f3 p2 = mk(pos.x + z, pos.y, pos.z);
        unsigned long long k2 = 0;
        for (int c = 0; c < P.ncl; c += 4) {
          const unsigned long long b0 = cluster_may_hit_mask(p2, dir, clus[c]) & hm;
          const unsigned long long b1 = cluster_may_hit_mask(p2, dir, clus[c + 1]) & hm;
          const unsigned long long b2 = cluster_may_hit_mask(p2, dir, clus[c + 2]) & hm;
          const unsigned long long b3 = cluster_may_hit_mask(p2, dir, clus[c + 3]) & hm;
          unsigned nib = (b0 ? 16u : 0u) | (b1 ? 32u : 0u) | (b2 ? 64u : 0u) | (b3 ? 128u : 0u);
          asm("" : "+s"(nib));
          k2 |= (unsigned long long)(nib >> 4) << c;
        }
        if (k2 == 0x123456789abcdefull) t = 1.0f;
      }
      for (int w = 0; w < nwords; ++w) {
        unsigned long long m = clm[w];
        // the kept clusters' member words, up to four requested per round trip (a repeated index
        // when fewer are left: the same word OR-ed twice)
        for (unsigned long long k2 = kc; k2;) {
          const int a = pop_lowest(k2);
          const int b = k2 ? pop_lowest(k2) : a;
          const int e = k2 ? pop_lowest(k2) : a;
          const int f = k2 ? pop_lowest(k2) : a;
          m |= clm[(size_t)(1 + a) * kClusterWords + w] | clm[(size_t)(1 + b) * kClusterWords + w] |
               clm[(size_t)(1 + e) * kClusterWords + w] | clm[(size_t)(1 + f) * kClusterWords + w];
        }
        exec_tests += (unsigned long long)__popcll(m);
        if (has) {
          // (streaming the word's 4-sphere groups with a per-nibble skip, or loading 4 survivors
          // per wait, were slower: configs d / e +1.2% / +0% and +0% / +5%, r03f / r03i)
          if (ABL == 1) {  // instruction-budget ablation: the cluster rounds' tests twice
            float z, t2 = -1.0f;
            int i2 = -1;
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            for (unsigned long long m2 = m; m2;) {
              const int i = (w << 6) + pop_lowest(m2);
              sphere_candidate(mk(pos.x + z, pos.y, pos.z), dir, geo[i], i, 0.0001f, t2, i2);
            }
            if (i2 == 0x7fffffff) t = t2;
          }
          // (the word's sphere pointer hoisted and the row index unsigned: the row's scalar load takes
          // it as a 32-bit byte offset instead of a sign-extended 64-bit address, 3 scalar
          // instructions fewer per survivor)
          const float4* const gw = geo + (w << 6);
          while (m) {
            const unsigned j = (unsigned)pop_lowest(m);
            sphere_candidate(pos, dir, gw[j], (w << 6) + (int)j, 0.0001f, t, ind);
          }
        }
      }
      if (has) {
        if (PL) plane_pass<RC>(P, pos, dir, 0.0001f, t, ind);
        ++nseg;
        has = shade(ind, t, pos, dir, hemi, rr, rg, rb, depth, item, false);
        depth -= 1;
      }
    } else if (has) {
      float t;
      int ind = closest_hit_pf(geo, nobj, pos, dir, 0.0001f, t);  // 4-sphere scalar groups (pf2: +0.9%)
      if (PL) plane_pass<RC>(P, pos, dir, 0.0001f, t, ind);
      if (ABL == 1) {  // timing ablation: the bounce tests twice
        float z, t2;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        int i2 = closest_hit_pf(geo, nobj, mk(pos.x + z, pos.y, pos.z), dir, 0.0001f, t2);
        if (i2 == 0x7fffffff) t = t2;
      }
      ++nseg;
      has = shade(ind, t, pos, dir, hemi, rr, rg, rb, depth, item, false);
      depth -= 1;
    }
    if (ABL == 8) tsec[6] += 1;
    lap(3);
  }
  lap(2);

  if (cnts && !kLaps && ABL != 7) {
    unsigned sg = wave_sum(nseg);
    if (lane == 0) {
      unsigned long long* c = cnts + (blockIdx.x & (kCounterSlots - 1));
      atomicAdd(&c[0 * kCounterSlots], (unsigned long long)total);
      atomicAdd(&c[1 * kCounterSlots], (unsigned long long)sg);
      atomicAdd(&c[3 * kCounterSlots], (unsigned long long)sg * (unsigned long long)nobj);
      atomicAdd(&c[4 * kCounterSlots], 64ull * exec_tests);
    }
  }
  __syncthreads();

  // ---- sample combine in aa order (ao_compute.glsl:303-339) ----------------------------
  for (int lp = lane; lp < np; lp += 64) {
    int x, y;
    pool_xy(lp, x, y);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    const float* ps = sres + lp * spp;
    if (SPPC % 4 == 0 && SPPC > 0) {
      // spp a multiple of 4 (constant): the pixel's samples read 4 at a time (ds_read_b128;
      // 16-byte aligned: lp * spp and NS are multiples of 4), summed in the same aa order
#pragma unroll 1
      for (int k = 0; k < SPPC; k += 4) {
        const float4 a = *(const float4*)(ps + k), g = *(const float4*)(ps + NS + k),
                     c = *(const float4*)(ps + 2 * NS + k);
        sr = sr + a.x; sr = sr + a.y; sr = sr + a.z; sr = sr + a.w;
        sg = sg + g.x; sg = sg + g.y; sg = sg + g.z; sg = sg + g.w;
        sb = sb + c.x; sb = sb + c.y; sb = sb + c.z; sb = sb + c.w;
      }
    } else {
#pragma unroll 1
      for (int k = 0; k < spp; ++k) {
        sr = sr + ps[k]; sg = sg + ps[NS + k]; sb = sb + ps[2 * NS + k];
      }
    }
    const int st = pstop[lp];
    const float ystop = st < 0 ? -1.0f : (float)(st & 0xffff);
    const float fa = (float)spp;
    const size_t off = (size_t)(y - P.band_row0) * W + x;
    const int kind = pkind[lp];
    float4 d;
    if (kind == PRIM_HIT) {
      float4 r0 = prec[lp];
      d = make_float4(r0.w, 0.0f, 0.0f, 1.0f);
      nrm_store(f_nrm, dep_plane(P), off, make_float4(r0.x, r0.y, r0.z, 1.0f));
    } else if (kind == PRIM_MISS) {
      d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      nrm_store(f_nrm, dep_plane(P), off, d);
    } else {  // stale: the slot's previous normal / depth (an emissive first hit writes neither)
      d = dep_load(f_dep_prev, dep_plane(P), off);
      if (f_nrm_prev != f_nrm) nrm_store(f_nrm, dep_plane(P), off, nrm_load(f_nrm_prev, dep_plane(P), off));
    }
    if (ystop >= 0.0f) d.y = ystop;
    d.x = d.x / fa; d.y = d.y / fa; d.z = d.z / fa; d.w = d.w / fa;
    dep_store(f_dep, dep_plane(P), off, d);
    store_color(P, f_out, f_img, x, y, gamma_out(sr / fa, sg / fa, sb / fa));
  }
  if ((kLaps || ABL == 7) && cnts && lane == 0) {
    lap(4);
    unsigned long long* c = cnts + (blockIdx.x & (kCounterSlots - 1));
    for (int k = 0; k < 8; ++k) atomicAdd(&c[k * kCounterSlots], tsec[k]);
  }
}

// (the streaming AO kernel of rounds 1-2, rejected in DESIGN.md §5, was removed in round 2)

// ---------------------------------------------------------------------------------------
// mode 1 pass 2 — aop_postprocessing.glsl:57-208, with the documented snapshot semantics:
// neighbours read `raw` (slot f before filtering); right iff x+1<W, left iff x>0,
// up iff y+1<H, down iff y>=2.  Output goes to out_pix (the shim swaps it into slot f).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void post_pixel(const FrameParams& P, int x, int y, unsigned& filtered, unsigned& visited,
                                           unsigned& accepted);

// XCD-local tile order: workgroups are dealt round-robin to the 8 XCDs (linear block id L on
// XCD L mod 8), each with its own L2, so in plain row-major order horizontally adjacent tiles
// sit on different XCDs and every tile's left / right neighbour columns (whole 128-B lines of
// raw, normals and depth) are fetched into a second L2.  Here the tiles are cut into runs of R
// consecutive tiles in row-major order and the runs are dealt round-robin to the XCDs, so most
// left / right neighbour lines were just brought into the tile's own L2 by the tile before it.
// The host picks R (launch_params: a divisor of gx / 8 when gx is a multiple of 8, so the tile
// below a tile is on its XCD too; >= 4).  Runs must stay short: every XCD has to take an equal
// share of every part of the frame, since sky costs far less than ground (one contiguous band
// per XCD cut the bytes by 19% but made the launch 43% slower; runs of 1/8 row, 11% slower).
// L -> run (L / 8 / R) * 8 + L mod 8, offset (L / 8) mod R: a bijection on the first multiple
// of 8R tiles; the rest keep their order.
//
// Round 4: when the host finds super-tiles of SX x SY blocks that tile the grid (launch_params:
// SX, SY in {4, 2} dividing gx, gy), each XCD takes whole super-tiles, dealt round-robin (row-major
// blocks inside), so a block's upper and lower neighbour rows are mostly in its own L2 too:
// config (d) post-process PMC 1.085 -> 1.044x the byte model, per-launch and pipelined-frame
// times unchanged (profiles/r04o_ab_post_super_tiles.txt; 4 x 12: 1.035x, 2 x 6: 1.052x).
// L -> super-tile (L / 8 / SS) * 8 + L mod 8, block (L / 8) mod SS for the first multiple of 8
// super-tiles; the rest in order: a bijection.
__device__ __forceinline__ void xcd_tile(unsigned R, unsigned SX, unsigned SY, unsigned& bx, unsigned& by) {
  if (SX * SY > 1) {
    const unsigned gx = gridDim.x, L = blockIdx.x + blockIdx.y * gx, SS = SX * SY;
    const unsigned gsx = gx / SX, Q = gsx * (gridDim.y / SY), M = Q / 8 * 8;
    unsigned q, o;
    if (L < M * SS) {
      const unsigned j = L >> 3;
      q = (j / SS) * 8 + (L & 7u);
      o = j % SS;
    } else {
      const unsigned L2 = L - M * SS;
      q = M + L2 / SS;
      o = L2 % SS;
    }
    bx = (q % gsx) * SX + o % SX;
    by = (q / gsx) * SY + o / SX;
    return;
  }
  const unsigned gx = gridDim.x, n = gx * gridDim.y, L = blockIdx.x + blockIdx.y * gx;
  const unsigned M = R ? n / (8 * R) * (8 * R) : 0;
  unsigned t = L;
  if (L < M) {
    const unsigned j = L >> 3;
    t = ((j / R) * 8 + (L & 7u)) * R + j % R;
  }
  by = t / gx;
  bx = t - by * gx;
}

// Post-process tile shape: a wave covers kPostWX x (64 / kPostWX) pixels, a block kPostBWX x
// kPostBWY waves (RT_POST_* overrides: A/B builds).  Round 4: a wave is one 64-pixel row segment
// and a block 64 x 4 pixels (was 8 x 8 waves in 16 x 16 blocks): a wave's loads of an array are
// then whole contiguous lines (1 KiB of colour, 768 B of normals, 512 B of depth), its left /
// right neighbours are its own lanes' lines but for the two edge pixels, and the up / down rows
// are the block's other waves'.  Config (d): 0.350 -> 0.300 ms per launch, same process
// (128 x 2 blocks 0.317, row-major tile order 0.321; profiles/r04d_ab_post.txt)
#ifndef RT_POST_WX
#define RT_POST_WX 64
#endif
#ifndef RT_POST_BWX
#define RT_POST_BWX 1
#endif
#ifndef RT_POST_BWY
#define RT_POST_BWY 4
#endif
constexpr int kPostWX = RT_POST_WX, kPostWY = 64 / RT_POST_WX, kPostBWX = RT_POST_BWX, kPostBWY = RT_POST_BWY;
constexpr int kPostTileW = kPostWX * kPostBWX, kPostTileH = kPostWY * kPostBWY;
static_assert(kPostWX * kPostWY == 64 && kPostBWX * kPostBWY * 64 == kBlock, "post tile shape");

__global__ __launch_bounds__(kBlock) void post_kernel(FrameParams P) {
  int x, y;
  unsigned bx, by;
  xcd_tile((unsigned)P.tile_run, (unsigned)P.post_sx, (unsigned)P.post_sy, bx, by);
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = (int)bx * kPostTileW + (wave % kPostBWX) * kPostWX + lane % kPostWX;
    y = P.trace_row0 + (int)by * kPostTileH + (wave / kPostBWX) * kPostWY + lane / kPostWX;
  }
  const bool active = x < P.W && y < P.trace_row0 + P.trace_rows;
  unsigned filtered = 0, visited = 0, accepted = 0;
  if (active) post_pixel(P, x, y, filtered, visited, accepted);
  if (P.counters) {
    unsigned n = wave_sum(filtered), v = wave_sum(visited), a = wave_sum(accepted);
    if ((threadIdx.x & 63) == 0) {
      unsigned long long* c = P.counters + ((blockIdx.x * 4 + blockIdx.y * 4 * gridDim.x + (threadIdx.x >> 6)) &
                                            (kCounterSlots - 1));
      atomicAdd(&c[5 * kCounterSlots], (unsigned long long)n);
      atomicAdd(&c[6 * kCounterSlots], (unsigned long long)v);
      atomicAdd(&c[7 * kCounterSlots], (unsigned long long)a);
    }
  }
}

// History slots read ahead of the acceptance test (see post_pixel).  1: the next slot's keys and
// colour are in flight while a slot is tested.  2 needs 76 VGPRs, more than the 72 an AO wave
// holds, so a post-process wave no longer fits in the registers one retiring AO wave frees and
// pipelined frames got 8% slower (profiles/r03s_ab_post_prefetch.txt).
constexpr int kPostAhead = 1;
struct HistSlot {
  f3 n;
  float2 d;
  float4 p;
};
__device__ __forceinline__ HistSlot hist_load(const FrameParams& P, int cf, size_t off) {
  HistSlot h;
  h.n = nrm_load_xyz(P.hist_nrm[cf], off);
  h.d = dep_load_xy(P.hist_dep[cf], off);
  h.p = P.hist_pix[cf][off];
  return h;
}

__device__ __forceinline__ void post_pixel(const FrameParams& P, int x, int y, unsigned& filtered, unsigned& visited,
                                           unsigned& accepted) {
  const int W = P.W, f = P.frame, F = P.F;
  const size_t off = (size_t)(y - P.band_row0) * W + x;
  float4 color = P.raw[off];
  const size_t np = dep_plane(P);  // normals: xyz plane + w plane (nrm_store)
  if (nrm_load_w(P.nrm, np, off) > 0.99f) {
    filtered = 1;
    // Memory round trips, not bytes, are what this kernel costs in the pipelined frame: there it
    // runs beside the next frame's AO pass, and each resident post-process wave holds registers
    // an AO wave could use for as long as it waits on memory.  So the neighbours are requested in
    // one round trip, and history slots f-1, f-2, ... kPostAhead ahead of the acceptance test with
    // keys and colour together (the colour of the slot that fails is read and dropped): ~F + 2
    // round trips per filtered pixel instead of ~2F + 9 (pipelined frames 2.368 -> 2.305 ms,
    // profiles/r03u_ab_post_round_trips.txt).  The arithmetic is the reference's, in its order.
    const float2 cd = dep_load_xy(P.dep, off);
    const f3 nv = nrm_load_xyz(P.nrm, off);
    const float nd = cd.x, nb = cd.y;
    float4 acc = color;
    float den = 1.0f;
    const int band_end = P.band_row0 + P.band_rows;
    // GLSL order: up, down, left, right (line 173).  Every neighbour's flag, keys and colour are
    // requested together (an absent neighbour reads the pixel itself and is dropped).
    {
      size_t o[4];
      bool pr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int xx = x + (k == 2 ? -1 : (k == 3 ? 1 : 0));
        int yy = y + (k == 0 ? 1 : (k == 1 ? -1 : 0));
        bool present = (k == 0) ? (y + 1 < P.H) : (k == 1) ? (y >= 2) : (k == 2) ? (x > 0) : (x + 1 < W);
        pr[k] = present && yy >= P.band_row0 && yy < band_end;
        const int xc = pr[k] ? xx : x, yc = pr[k] ? yy : y;  // (a select, not a branch on a shared load)
        o[k] = (size_t)(unsigned)((yc - P.band_row0) * W + xc);
      }
      float wn[4];
      f3 nn[4];
      float2 dd[4];
      float4 rv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wn[k] = nrm_load_w(P.nrm, np, o[k]);
        nn[k] = nrm_load_xyz(P.nrm, o[k]);
        dd[k] = dep_load_xy(P.dep, o[k]);
        rv[k] = P.raw[o[k]];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // the neighbour weight (aop_postprocessing.glsl:82-171: 1 for a sky neighbour), branch-free
        // so the compiler keeps the loads above together
        const float normal_dot = dot(nv, nn[k]);
        const float depth_diff = 1.0f - gclamp(fabsf(nd - dd[k].x), 0.0f, 1.0f);
        const float bounces_diff = 1.0f - gclamp(fabsf(nb - dd[k].y) / 1.7f, 0.0f, 1.0f);
        const float wf = normal_dot * depth_diff * bounces_diff + 0.2f;
        const float wk = pr[k] ? (wn[k] < 0.001f ? 1.0f : wf) : 0.0f;
        const float4 v = pr[k] ? rv[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        acc.x = acc.x + wk * v.x; acc.y = acc.y + wk * v.y;
        acc.z = acc.z + wk * v.z; acc.w = acc.w + wk * v.w;
        den = den + wk;
      }
    }
    color = make_float4(acc.x / den, acc.y / den, acc.z / den, acc.w / den);
    // temporal, lines 177-201
    HistSlot ring[kPostAhead];
    int cf = f;
    int issued = 0;
#pragma unroll
    for (int k = 0; k < kPostAhead; ++k)
      if (k < F - 1) {
        cf = cf == 0 ? F - 1 : cf - 1;
        ring[k] = hist_load(P, cf, off);
        ++issued;
      }
    float4 cs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float denominator = 0.9f;
    for (int i = 1; i < F; ++i) {
      const HistSlot h = ring[0];
#pragma unroll
      for (int k = 0; k + 1 < kPostAhead; ++k) ring[k] = ring[k + 1];
      if (issued < F - 1) {  // slot f-i-kPostAhead, in flight while slot f-i is tested
        cf = cf == 0 ? F - 1 : cf - 1;
        ring[kPostAhead - 1] = hist_load(P, cf, off);
        ++issued;
      }
      float normal_dot = dot(nv, h.n);
      float depth_diff = 1.0f - gclamp(fabsf(nd - h.d.x), 0.0f, 1.0f);
      float bounces_diff = 1.0f - gclamp(fabsf(nb - h.d.y) / 1.7f, 0.0f, 1.0f);
      float coeff = normal_dot * depth_diff * bounces_diff;
      ++visited;
      if (!(coeff > 0.85f)) break;
      ++accepted;
      cs.x = cs.x + coeff * h.p.x; cs.y = cs.y + coeff * h.p.y;
      cs.z = cs.z + coeff * h.p.z; cs.w = cs.w + coeff * h.p.w;
      denominator = denominator + coeff;
    }
    color = make_float4((color.x * 0.9f + cs.x) / denominator, (color.y * 0.9f + cs.y) / denominator,
                        (color.z * 0.9f + cs.z) / denominator, (color.w * 0.9f + cs.w) / denominator);
  }
  store_color(P, x, y, color);
}

// ---------------------------------------------------------------------------------------
// math self-test
// ---------------------------------------------------------------------------------------
// The view of the cull self-tests (RT_MATH_CULL_CAMERA / _PLANE): the FrameParams fields that
// pool_cone_f and primary_dir read, from a[3..13] = llc_minus_campos, horizontal, vertical, W, H.
__device__ __forceinline__ void selftest_view(FrameParams& P, const float* a) {
  P.lx = a[3]; P.ly = a[4]; P.lz = a[5];
  P.hx = a[6]; P.hy = a[7]; P.hz = a[8];
  P.vx = a[9]; P.vy = a[10]; P.vz = a[11];
  P.fW = a[12]; P.fH = a[13];
}

// Cases of the wave-per-case functions (their 64 lanes share ballots and DPP reductions).
__host__ __device__ constexpr bool selftest_wave_fn(int fn) { return fn == 14 || fn == 16; }

__global__ void selftest_kernel(int fn, const float* __restrict__ in, float* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (selftest_wave_fn(fn)) i >>= 6;  // one wave per case: the exit below is wave-uniform
  if (i >= n) return;
  switch (fn) {
    case 12: {  // camera-ray cone vs sphere, and the exact sphere test's forms
      const float* a = in + 24 * i;
      FrameParams P;
      selftest_view(P, a);
      const f3 cam = mk(a[0], a[1], a[2]);
      const float4 g = make_float4(a[20], a[21], a[22], a[23]);
      const ConeF cone = pool_cone_f(P, (int)a[14], (int)a[15], (int)a[16], (int)a[17]);
      const f3 dir = primary_dir(P, a[18], a[19]);
      // the sphere's camera-relative row as rt_shim pack_header forms it
      const float px = cam.x - g.x, py = cam.y - g.y, pz = cam.z - g.z;
      const float4 q = make_float4(px, py, pz, fmaf(pz, pz, fmaf(py, py, px * px)));
      float t_ao = -1.0f, t_p = -1.0f;
      int ind = -1;
      sphere_candidate_rel(dir, q, g.w, 0, 0.0001f, t_ao, ind);
      sphere_candidate_rel(dir, q, g.w, 0, 0.0f, t_p, ind);
      float* o = out + 7 * i;
      o[0] = dir.x; o[1] = dir.y; o[2] = dir.z;
      o[3] = cone_misses_f(cone, g, cam.x, cam.y, cam.z) ? 1.0f : 0.0f;
      o[4] = sphere_eval(cam, dir, g);
      o[5] = t_ao;
      o[6] = t_p;
      break;
    }
    case 13: {  // camera-ray cone vs plane
      const float* a = in + 28 * i;
      FrameParams P;
      selftest_view(P, a);
      const f3 cam = mk(a[0], a[1], a[2]);
      const float4 pa = make_float4(a[20], a[21], a[22], a[23]), pb = make_float4(a[24], a[25], a[26], a[27]);
      const ConeF cone = pool_cone_f(P, (int)a[14], (int)a[15], (int)a[16], (int)a[17]);
      const f3 dir = primary_dir(P, a[18], a[19]);
      out[2 * i] = plane_cone_misses(cone, pa, pb, cam) ? 1.0f : 0.0f;
      out[2 * i + 1] = plane_eval(cam, dir, pa, pb);
      break;
    }
    case 14: {  // first-bounce cone of one wave's rays vs sphere, and the per-ray pre-test
      const int lane = threadIdx.x & 63;
      const float* a = in + 452 * i;
      const float* q = a + 4 + 7 * lane;
      const float4 g = make_float4(a[0], a[1], a[2], a[3]);
      const f3 p = mk(q[0], q[1], q[2]), d = mk(q[3], q[4], q[5]);
      const bool live = q[6] != 0.0f;
      const unsigned long long lm = __ballot(live);
      float miss = 0.0f, keep = 1.0f, pass = 0.0f, t = -1.0f, t_if = -1.0f;
      if (lm != 0) {  // (the kernel builds no cone for a batch without live lanes)
        const ConeB cb = bounce_cone(live, p, d, lm);
        float4 pt;
        miss = bounce_cone_misses(cb, g) ? 1.0f : 0.0f;
        keep = bounce_cone_keep_pt(cb, g, pt) ? 1.0f : 0.0f;
        f3 tdir = d;  // NaN on the lanes that are not live, as in ao_batch_kernel
        if (!live) tdir = mk(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
        pass = fmaf(tdir.z, pt.z, fmaf(tdir.y, pt.y, tdir.x * pt.x)) >= pt.w ? 1.0f : 0.0f;
        int ind = -1, ind_if = -1;
        sphere_candidate(p, d, g, 0, 0.0001f, t, ind);
        // the form the batched first bounce runs: only the lanes whose pre-test passed may accept
        const unsigned long long pm = __builtin_amdgcn_ballot_w64(pass != 0.0f);
        if (pm != 0) sphere_candidate_if(p, d, g, 0, 0.0001f, t_if, ind_if, pm);
      }
      float* o = out + 320 * i + 5 * lane;
      o[0] = miss; o[1] = keep; o[2] = pass; o[3] = t; o[4] = t_if;
      break;
    }
    case 15: {  // cluster ball vs ray, both forms, and a member's exact test
      const float* a = in + 14 * i;
      const f3 p = mk(a[0], a[1], a[2]), d = mk(a[3], a[4], a[5]);
      const float4 cb = make_float4(a[6], a[7], a[8], a[9]), g = make_float4(a[10], a[11], a[12], a[13]);
      const unsigned long long m = cluster_may_hit_mask(p, d, cb);
      float t = -1.0f;
      int ind = -1;
      sphere_candidate(p, d, g, 0, 0.0001f, t, ind);
      out[3 * i] = cluster_may_hit(p, d, cb) ? 1.0f : 0.0f;
      out[3 * i + 1] = (m >> (threadIdx.x & 63)) & 1ull ? 1.0f : 0.0f;
      out[3 * i + 2] = t;
      break;
    }
    case 17: {  // the query tree's unit gate, node decision and member test (thr 0, from t = -1)
      const float* a = in + 14 * i;
      const f3 p = mk(a[0], a[1], a[2]), d = mk(a[3], a[4], a[5]);
      const float4 cb = make_float4(a[6], a[7], a[8], a[9]), g = make_float4(a[10], a[11], a[12], a[13]);
      const bool gate = unit_gate(d);
      float t = -1.0f;
      int ind = -1;
      tree_sphere(p, d, g, 0, 0.0f, t, ind);
      out[3 * i] = gate ? 1.0f : 0.0f;
      out[3 * i + 1] = tree_may_hit(gate, p, d, cb) ? 1.0f : 0.0f;
      out[3 * i + 2] = t;
      break;
    }
    case 16: {  // shadow cone at the light over one wave's shaded points vs sphere
      const int lane = threadIdx.x & 63;
      const float* a = in + 263 * i;
      const float* q = a + 7 + 4 * lane;
      const f3 light = mk(a[0], a[1], a[2]), pos = mk(q[0], q[1], q[2]);
      const float4 g = make_float4(a[3], a[4], a[5], a[6]);
      const bool need = q[3] != 0.0f;
      // shadow_lit_cone's set-up
      const f3 lv = light - pos;
      const f3 l = normalize(lv);
      const float len = sqrtf(dot(lv, lv));
      const f3 np = pos + 0.01f * l;
      const double dlen = (double)len;
      float lmax;
      const ConeF cone = shadow_cone(need, l, len, lmax);
      const bool wide = !(cone.ct > 0.05f);
      out[128 * i + 2 * lane] = shadow_cone_keeps(cone, wide, g, light, lmax) ? 1.0f : 0.0f;
      out[128 * i + 2 * lane + 1] = shadow_occludes(sphere_eval_shadow(np, l, g), l, dlen) ? 1.0f : 0.0f;
      break;
    }
    case 0: out[i] = det_sin(in[i]); break;
    case 9: out[i] = det_sin(__uint_as_float(__float_as_uint(in[0]) + (unsigned)i)); break;  // bit patterns in[0].., wrapping
    case 1: out[i] = grandom(in[2 * i], in[2 * i + 1]); break;
    case 2: out[i] = sqrt_rn(in[i]); break;
    case 6: {  // exhaustive sqrt_rn == sqrtf over bit patterns [i*per, (i+1)*per) of [0, 0x7f800000]
      const unsigned per = (unsigned)in[0];
      unsigned bad = 0;
      for (unsigned k = 0; k < per; ++k) {
        unsigned long long u = (unsigned long long)i * per + k;
        if (u > 0x7f800000ull) break;
        float x = __uint_as_float((unsigned)u);
        bad += __float_as_uint(sqrt_rn(x)) != __float_as_uint(sqrtf(x));
      }
      out[i] = (float)bad;
      break;
    }
    case 7: {  // exhaustive inv_len_rn == 1/sqrtf over [0, 0x7f800000]; rcp_rn_normal == 1/x on [2^-126, 2^126]
      const unsigned per = (unsigned)in[0];
      unsigned bad = 0;
      for (unsigned k = 0; k < per; ++k) {
        unsigned long long u = (unsigned long long)i * per + k;
        if (u > 0x7f800000ull) break;
        float x = __uint_as_float((unsigned)u);
        bad += __float_as_uint(inv_len_rn(x)) != __float_as_uint(1.0f / sqrtf(x));
        if (u >= 0x00800000ull && u <= 0x7e800000ull) bad += __float_as_uint(rcp_rn_normal(x)) != __float_as_uint(1.0f / x);
      }
      out[i] = (float)bad;
      break;
    }
    case 8: {  // exhaustive sqrt_rn_tail contract over [0, 0x7f7fffff]: == sqrtf on [2^-96, FLT_MAX], in [0, 2^-47] below
      const unsigned per = (unsigned)in[0];
      unsigned bad = 0;
      for (unsigned k = 0; k < per; ++k) {
        unsigned long long u = (unsigned long long)i * per + k;
        if (u > 0x7f7fffffull) break;
        float x = __uint_as_float((unsigned)u);
        const float s = sqrt_rn_tail(x);
        if (u >= 0x0f800000ull) bad += __float_as_uint(s) != __float_as_uint(sqrtf(x));
        else bad += !(s >= 0.0f && s <= 0x1p-47f);
        bad += __float_as_uint(sqrt_rn_tail_inf(x)) != __float_as_uint(s);  // the same root on every finite float
      }
      out[i] = (float)bad;
      break;
    }
    case 3: out[i] = in[2 * i] / in[2 * i + 1]; break;
    case 11: {  // the exception table against this build's device code: entry i is an input whose
      // binary64 sin (det_sin_rare's sin_binary64) is ambiguous to round, so its table value is used
      if (i < (size_t)kSinTableN) {
        const float x = __uint_as_float(kSinTableX[i]);
        out[2 * i] = sin_ambiguous(sin_binary64(x)) ? 1.0f : 0.0f;
        out[2 * i + 1] = __uint_as_float(kSinTableX[i]);
      } else {
        out[2 * i] = -1.0f;
        out[2 * i + 1] = 0.0f;
      }
      break;
    }
    case 10: {  // shadow_lit_cone's per-ray set-up and occluder test for one (light - pos, t)
      const f3 lv = mk(in[4 * i], in[4 * i + 1], in[4 * i + 2]);
      const f3 l = normalize(lv);
      const float len = sqrtf(dot(lv, lv));
      const bool occ = shadow_occludes(in[4 * i + 3], l, (double)len);
      out[5 * i] = l.x; out[5 * i + 1] = l.y; out[5 * i + 2] = l.z; out[5 * i + 3] = len;
      out[5 * i + 4] = occ ? 1.0f : 0.0f;
      break;
    }
    case 4: {
      f3 v = normalize(mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
      out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z;
      break;
    }
    case 5: {
      const float* a = in + 10 * i;
      out[i] = sphere_eval(mk(a[0], a[1], a[2]), mk(a[3], a[4], a[5]), make_float4(a[6], a[7], a[8], a[9]));
      break;
    }
    default: break;
  }
}

size_t shapes_lds_bytes(const FrameParams& p) { return (size_t)4 * p.nobj * sizeof(float4); }
size_t tab_lds_bytes(const FrameParams& p) { return (size_t)5 * (p.nobj > 0 ? p.nobj : 1) * sizeof(float4); }

}  // namespace

// The primary-ray cull of ao_batch_kernel's pool start for every pool of a launch, kept: row pb of
// `table` holds pool pb's cmask words (pb = the pool index after the kernel's pool_rot mapping,
// i.e. the pool of pixels [pb TP, pb TP + np), so the table does not depend on the rotation).
// One wave per pool and the kernel's own expressions, operand for operand (this file is built with
// -ffp-contract=off), so the masks are the ones the pool would have computed, bit for bit.
//
// FRAMES: the pool's sort frame too, in front of the masks (FrameParams::cull_frames).  The ray is
// the one prepare() forms for sample 0 (no jitter) of the pool's middle pixel, so while the masks
// hold it holds; it meets the pool's surviving spheres in ascending order as prepare() does.  n0 is
// the hit sphere's normal there, or the reversed ray when the middle pixel sees sky (a silhouette
// pool); e1 = normalize(n0 x ref), e2 = n0 x e1, ref the x axis unless |n0.x| >= 0.9, then the y
// axis.  Raw v_rsq: the frame orders the pool's samples and nothing else.  Every lane computes the
// same values (one uniform ray), lane 0 stores them.
//
// The pool list (rt_kernels.h ao_pool_list_bytes) is written from the filled masks by two further
// launches of the FRAMES kernel with P.cull_frames as a mode word (launch_pool_list), block c over
// chunk c of kPoolListChunk pools, 64 pools a step, one per lane.  A pool is sky when its masks are
// all zero, the ncull == 0 of ao_batch_kernel's sky exit.  Mode 1: the chunk's non-sky count.  Mode
// 2: the block sums the counts of the chunks before its own, then a pool's row index is that sum
// plus the non-sky pools before it in the chunk (ballots), and its sky index the pools before it
// less those: both lists ascend in pb whatever order the blocks run in.  The last block writes
// the two counts.  (xf, yf, np): ao_batch_kernel's pool start, expression for expression.
__device__ __forceinline__ void pool_list_build(const FrameParams& P, unsigned long long* table, bool write) {
  const int spp = P.spp, W = P.W;
  const int TP = kPool / spp > 0 ? kPool / spp : 1;
  const unsigned lane = threadIdx.x, chunk = blockIdx.x;
  const long long npix = (long long)P.trace_rows * W;
  const unsigned pools = (unsigned)((npix + TP - 1) / TP), nwords = (unsigned)(P.nobj + 63) >> 6;
  char* const base = (char*)table - ao_cull_frame_bytes(pools) - ao_pool_list_bytes(pools);
  int4* const rows = (int4*)base;
  unsigned* const sky_end = (unsigned*)(base + 16 * (size_t)pools);
  unsigned* const counts = sky_end;  // the chunk counts start where the rows' 16 x pools bytes end
  unsigned before = 0;  // non-sky pools in front of the step's 64
  if (write) {
    for (unsigned k = lane; k < chunk; k += 64) before += counts[k];
    before = wave_sum(before);
  }
  const unsigned first = chunk * (unsigned)kPoolListChunk;
  for (unsigned s = 0; s < (unsigned)kPoolListChunk && first + s < pools; s += 64) {
    const unsigned pb = first + s + lane;
    bool nonsky = false;
    if (pb < pools)
      for (unsigned w = 0; w < nwords; ++w) nonsky = nonsky || table[(size_t)pb * nwords + w] != 0;
    const unsigned long long m = __ballot(nonsky);
    if (write && pb < pools) {
      const unsigned at = before + (unsigned)__popcll(m & ((1ull << lane) - 1));
      if (nonsky) {
        const long long p0 = (long long)pb * TP;
        const int np = (int)(npix - p0 < TP ? npix - p0 : TP);
        const int yf = P.trace_row0 + (int)(p0 / W), xf = (int)(p0 % W);
        rows[at] = make_int4((int)pb, xf, yf, np);
      } else {
        sky_end[-1 - (long long)(pb - at)] = pb;
      }
    }
    before += (unsigned)__popcll(m);
  }
  if (lane != 0) return;
  if (!write) counts[chunk] = before;
  else if (chunk == gridDim.x - 1)
    *(int4*)((char*)table - ao_cull_frame_bytes(pools) - 16) = make_int4((int)before, (int)(pools - before), 0, 0);
}

template <bool FRAMES>
__global__ __launch_bounds__(64) void cull_fill_kernel(FrameParams P, const float4* __restrict__ geo,
                                                       unsigned long long* __restrict__ table) {
  if constexpr (FRAMES) {
    if (P.cull_frames != 0) {  // (wave-uniform) the pool list's build, not the fill
      pool_list_build(P, table, P.cull_frames == 2);
      return;
    }
  }
  const int spp = P.spp, W = P.W, nobj = P.nobj;
  const int TP = kPool / spp > 0 ? kPool / spp : 1;
  const int lane = threadIdx.x;
  const long long npix = (long long)P.trace_rows * W;
  const unsigned pb = blockIdx.x;
  const long long p0 = (long long)pb * TP;
  const int np = (int)(npix - p0 < TP ? npix - p0 : TP);
  const int yf = P.trace_row0 + (int)(p0 / W), xf = (int)(p0 % W);
  const int yl = P.trace_row0 + (int)((p0 + np - 1) / W), xl = (int)((p0 + np - 1) % W);
  const int nwords = (nobj + 63) >> 6;
  const ConeF cone = pool_cone_f(P, yf == yl ? xf : 0, yf == yl ? xl : W - 1, yf, yl);
  const f3 cam = mk(P.cx, P.cy, P.cz);
  f3 dir = cam;
  if (FRAMES) {  // pixel np / 2 of the pool, as the kernel's pool_xy and prepare() with aa == 0
    int x = xf + np / 2, y = yf;
    if (x >= W) {
      const int q = (int)((unsigned)x / (unsigned)W);
      y += q;
      x -= q * W;
    }
    dir = primary_dir(P, div_rn_by((float)x + 0.0f, P.fW, P.inv_W), div_rn_by((float)y + 0.0f, P.fH, P.inv_H));
  }
  float t = -1.0f;
  int ind = -1;
  for (int w = 0; w < nwords; ++w) {
    int i = (w << 6) + lane;
    bool keep = i < nobj && !cone_misses_f(cone, geo[i], P.cx, P.cy, P.cz);
    unsigned long long m = __ballot(keep);
    if (lane == 0) table[(size_t)pb * (unsigned)nwords + w] = m;
    if (FRAMES) {
      m = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
          (unsigned)__builtin_amdgcn_readfirstlane((unsigned)m);
      while (m) {
        const int j = pop_lowest(m);  // (j < 64 and bit j set only for (w << 6) + j < nobj)
        sphere_candidate(cam, dir, geo[(w << 6) + j], (w << 6) + j, 0.0001f, t, ind);
      }
    }
  }
  if (FRAMES) {
    f3 n0 = mk(-dir.x, -dir.y, -dir.z);
    if (ind >= 0) {  // (wave-uniform)
      const f3 v = (cam + t * dir) - xyz(geo[ind]);
      n0 = fast_rsq(dot(v, v)) * v;
    }
    // n0 x ref: ref = (1, 0, 0), or (0, 1, 0) when n0 is within 26 degrees of the x axis
    const bool ry = fabsf(n0.x) >= 0.9f;
    const f3 c = ry ? mk(-n0.z, 0.0f, n0.x) : mk(0.0f, n0.z, -n0.y);
    const f3 e1 = fast_rsq(dot(c, c)) * c;
    const f3 e2 = mk(n0.y * e1.z - n0.z * e1.y, n0.z * e1.x - n0.x * e1.z, n0.x * e1.y - n0.y * e1.x);
    if (lane == 0) {
      float4* const fr = (float4*)table - 2 * ((size_t)pb + 1);
      fr[0] = make_float4(e1.x, e1.y, e1.z, 0.0f);
      fr[1] = make_float4(e2.x, e2.y, e2.z, 0.0f);
    }
  }
}

// The launch log's entry for the kernel a launcher is about to launch (rt_kernels.h LaunchLog; only
// called with a log): the name as written, or built from the template arguments the launcher chose.
inline void note_launch(LaunchLog* log, const char* name) { log->names.emplace_back(name); }
template <class A0, class... A>
inline void note_launch(LaunchLog* log, const char* fmt, A0 a0, A... a) {
  char name[128];
  snprintf(name, sizeof name, fmt, a0, a...);
  log->names.emplace_back(name);
}
// hipLaunchKernelGGL(kernel, ...) with its log entry beside it: the name is written where the kernel
// is, so a branch cannot log one form and launch another (tests/test_kernel_census_cpu.py holds the
// names against the library's symbols)
#define RT_LAUNCH(log, name, kernel, ...)    \
  do {                                       \
    if (log) note_launch(log, name);         \
    hipLaunchKernelGGL(kernel, __VA_ARGS__); \
  } while (0)
#define RT_STR2(x) #x
#define RT_STR(x) RT_STR2(x)
#define RT_HYBW RT_STR(RT_HY_BW) ", " RT_STR(RT_HY_BW)  // kHyBW, kHyBW as a kernel name spells them

hipError_t launch_cull_fill(const FrameParams& p, unsigned long long* table, bool frames, hipStream_t stream, LaunchLog* log) {
  const long long pools = ao_pool_count(p.trace_rows, p.W, p.spp);
  if (pools <= 0 || p.nobj <= 0) return hipSuccess;
  const float4* const sph = p.shapes + sphere_table(p.S);
  FrameParams q = p;
  q.cull_frames = 0;  // (the FRAMES kernel's mode word: the fill)
  if (frames) RT_LAUNCH(log, "cull_fill_kernel<true>", cull_fill_kernel<true>, dim3((unsigned)pools), dim3(64), 0, stream, q, sph, table);
  else RT_LAUNCH(log, "cull_fill_kernel<false>", cull_fill_kernel<false>, dim3((unsigned)pools), dim3(64), 0, stream, q, sph, table);
  return hipGetLastError();
}

hipError_t launch_pool_list(const FrameParams& p, unsigned long long* table, hipStream_t stream) {
  const long long pools = ao_pool_count(p.trace_rows, p.W, p.spp);
  if (pools <= 0 || p.nobj <= 0) return hipSuccess;
  const dim3 grid((unsigned)((pools + kPoolListChunk - 1) / kPoolListChunk));
  FrameParams q = p;
  for (int mode = 1; mode <= 2; ++mode) {  // (not logged: part of the fill, whose entry launch_cull_fill made)
    q.cull_frames = mode;
    hipLaunchKernelGGL(cull_fill_kernel<true>, grid, dim3(64), 0, stream, q, p.shapes + sphere_table(p.S), table);
  }
  return hipGetLastError();
}

constexpr int kRefDepth = 20;  // RECURSION_DEPTH, ao_compute.glsl:9
// least spheres of a scene whose pools are sorted (RT_B1_SORT_MIN overrides: A/B builds)
#ifndef RT_B1_SORT_MIN
#define RT_B1_SORT_MIN 48
#endif
constexpr int kB1SortMinObj = RT_B1_SORT_MIN;

// The production AO configuration of a launch: AoProd<sppc, dc, flags>.
struct AoChoice {
  int sppc, dc;
  unsigned flags;  // AO_*
};
constexpr bool operator==(const AoChoice& a, const AoChoice& b) {
  return a.sppc == b.sppc && a.dc == b.dc && a.flags == b.flags;
}
// - spp 4 (the reference's AA), 16 (configs c/d) and 64 (config e; not with planes) have their own
//   instantiations: constant LDS offsets and it / spp, fewer scalar registers.
// - The reference's RECURSION_DEPTH with bounce-ray clusters (every all-sphere scene of 16..256
//   spheres) also has its own for spp 16 and 64: with the depth a constant and the rounds' plain
//   full-scan fallback compiled out, fewer scalar registers are spilled to vector lanes (each
//   reload is a v_readlane on the bounce rounds' path).
// - The pools are sorted in scenes without planes of at least kB1SortMinObj spheres (below, the
//   first bounce's cone keeps too few spheres for the sort to pay: 1920x1080, 16 spp, sorted
//   against unsorted +2.5% / +2% / +4% at 16 / 24 / 32 spheres, -2% at 48,
//   profiles/r07_ab_b1_sort_threshold.txt; plane scenes were not measured and stay unsorted).
// - Above kTailMaxObj spheres the sphere table does not fit the kernel's LDS rows (AO_WIDE).
// - Timed launches pass no counters: the counter code is compiled out.  A multi-frame launch
//   never has counters (rt_compute_frames checks).
// - A launch handed a table of its pools' cull masks (FrameParams::cull) loads them (AO_CULLC);
//   scenes with planes never are (their pmask has no table) and keep the in-kernel cull.
constexpr AoChoice ao_select(int spp, int D, int ncl, int nobj, int nplanes, bool counters, bool multi_frame,
                             bool cull_table) {
  const bool pl = nplanes > 0;
  const bool own = spp == 16 || spp == 4 || (spp == 64 && !pl);
  const bool clon = !pl && (spp == 16 || spp == 64) && D == kRefDepth && ncl > 0;
  return AoChoice{own ? spp : 0, clon ? kRefDepth : 0,
                  (pl ? AO_PL : 0u) | (clon ? AO_CLON : 0u) | (RT_B1_SORT && !pl && nobj >= kB1SortMinObj ? AO_SORT : 0u) |
                      (nobj > kTailMaxObj ? AO_WIDE : 0u) | (multi_frame ? AO_MF : counters ? AO_CNT : 0u) |
                      (cull_table && !pl ? AO_CULLC : 0u)};
}
// Rectangles in effect (nrects > 0 of the nplanes entries): the plane scene's choice with AO_RC.
constexpr AoChoice ao_select(int spp, int D, int ncl, int nobj, int nplanes, int nrects, bool counters, bool multi_frame,
                             bool cull_table) {
  const AoChoice c = ao_select(spp, D, ncl, nobj, nplanes, counters, multi_frame, cull_table);
  return AoChoice{c.sppc, c.dc, c.flags | (nplanes > 0 && nrects > 0 ? AO_RC : 0u)};
}
// The dispatch's regression test (derived from the launcher this function replaced).  Arguments:
// spp, D, ncl, nobj, nplanes, counters, multi-frame, cull table.
constexpr unsigned kSortBit = RT_B1_SORT ? AO_SORT : 0u;
// bench.py's configs, timed launch; (a) and (b) are Phong / hybrid scenes, never launched as AO
static_assert(ao_select(1, 20, 0, 4, 0, false, false, false) == AoChoice{0, 0, 0}, "a");
static_assert(ao_select(1, 20, 4, 16, 0, false, false, false) == AoChoice{0, 0, 0}, "b");
static_assert(ao_select(16, 20, 8, 64, 0, false, false, false) == AoChoice{16, 20, AO_CLON | kSortBit}, "c");
static_assert(ao_select(16, 20, 8, 64, 0, false, false, false) == AoChoice{16, 20, AO_CLON | kSortBit}, "d");
static_assert(ao_select(64, 20, 16, 256, 0, false, false, false) == AoChoice{64, 20, AO_CLON | kSortBit | AO_WIDE}, "e");
static_assert(ao_select(16, 20, 9, 65, 1, false, false, false) == AoChoice{16, 0, AO_PL}, "p");
static_assert(ao_select(16, 20, 9, 65, 0, false, false, false) == AoChoice{16, 20, AO_CLON | kSortBit}, "q");
static_assert(ao_select(16, 20, 0, 10, 1, false, false, false) == AoChoice{16, 0, AO_PL}, "s1");
static_assert(ao_select(4, 20, 0, 10, 1, false, false, false) == AoChoice{4, 0, AO_PL}, "ref");
// counters on; a multi-frame launch (its counters flag is ignored)
static_assert(ao_select(16, 20, 8, 64, 0, true, false, false) == AoChoice{16, 20, AO_CLON | kSortBit | AO_CNT}, "counters");
static_assert(ao_select(16, 20, 8, 64, 0, false, true, false) == AoChoice{16, 20, AO_CLON | kSortBit | AO_MF}, "multi-frame");
static_assert(ao_select(16, 20, 8, 64, 0, true, true, false) == AoChoice{16, 20, AO_CLON | kSortBit | AO_MF}, "multi-frame");
// just under and at kB1SortMinObj; at and above kTailMaxObj
static_assert(ao_select(16, 20, 6, kB1SortMinObj - 1, 0, false, false, false) == AoChoice{16, 20, AO_CLON}, "unsorted");
static_assert(ao_select(16, 20, 6, kB1SortMinObj, 0, false, false, false) == AoChoice{16, 20, AO_CLON | kSortBit}, "sorted");
static_assert(ao_select(64, 20, 12, kTailMaxObj, 0, false, false, false) == AoChoice{64, 20, AO_CLON | kSortBit}, "LDS table");
static_assert(ao_select(64, 20, 12, kTailMaxObj + 1, 0, false, false, false) == AoChoice{64, 20, AO_CLON | kSortBit | AO_WIDE}, "wide");
// another depth, no clusters, other spp, planes with spp 64
static_assert(ao_select(16, 10, 8, 64, 0, false, false, false) == AoChoice{16, 0, kSortBit}, "depth 10");
static_assert(ao_select(64, 20, 0, 300, 0, false, false, false) == AoChoice{64, 0, kSortBit | AO_WIDE}, "no clusters");
static_assert(ao_select(4, 20, 8, 64, 0, false, false, false) == AoChoice{4, 0, kSortBit}, "spp 4");
static_assert(ao_select(8, 20, 8, 64, 0, true, false, false) == AoChoice{0, 0, kSortBit | AO_CNT}, "spp 8");
static_assert(ao_select(64, 20, 8, 200, 2, false, false, false) == AoChoice{0, 0, AO_PL | AO_WIDE}, "planes, spp 64");
// with a cull table: the same choice plus AO_CULLC, in every form but the plane scenes'
static_assert(ao_select(16, 20, 8, 64, 0, false, false, true) == AoChoice{16, 20, AO_CLON | kSortBit | AO_CULLC}, "c, d cached");
static_assert(ao_select(64, 20, 16, 256, 0, false, false, true) == AoChoice{64, 20, AO_CLON | kSortBit | AO_WIDE | AO_CULLC},
              "e cached");
static_assert(ao_select(16, 20, 8, 64, 0, true, false, true) == AoChoice{16, 20, AO_CLON | kSortBit | AO_CNT | AO_CULLC},
              "counters cached");
static_assert(ao_select(16, 20, 8, 64, 0, false, true, true) == AoChoice{16, 20, AO_CLON | kSortBit | AO_MF | AO_CULLC},
              "multi-frame cached");
static_assert(ao_select(8, 20, 8, 64, 0, false, false, true) == AoChoice{0, 0, kSortBit | AO_CULLC}, "spp 8 cached");
// the frame key: the cached, sorted, timed forms (multi-frame included); every other form the octant key
static_assert(ao_sorts_by_frame(ao_select(16, 20, 8, 64, 0, false, false, true).flags) == (kSortBit != 0), "c, d cached");
static_assert(ao_sorts_by_frame(ao_select(64, 20, 16, 256, 0, false, false, true).flags) == (kSortBit != 0), "e cached");
static_assert(ao_sorts_by_frame(ao_select(16, 20, 8, 64, 0, false, true, true).flags) == (kSortBit != 0), "multi-frame cached");
static_assert(!ao_sorts_by_frame(ao_select(16, 20, 8, 64, 0, true, false, true).flags), "counters cached: octants");
static_assert(!ao_sorts_by_frame(ao_select(16, 20, 8, 64, 0, false, false, false).flags), "uncached: octants");
static_assert(!ao_sorts_by_frame(ao_select(16, 20, 6, kB1SortMinObj - 1, 0, false, false, true).flags), "unsorted");
static_assert(!ao_sorts_by_frame(ao_select(16, 20, 9, 65, 1, false, false, true).flags), "planes");
static_assert(ao_select(16, 20, 9, 65, 1, false, false, true) == AoChoice{16, 0, AO_PL}, "p: never cached");
static_assert(ao_select(4, 20, 0, 10, 1, false, false, true) == AoChoice{4, 0, AO_PL}, "ref: never cached");

// rectangles: spp, D, ncl, nobj, nplanes, nrects, counters, multi-frame, cull table; the plane rows with AO_RC,
// never cached, never sorted; no rectangle in effect: the choice above
static_assert(ao_select(16, 20, 9, 65, 1, 1, false, false, false) == AoChoice{16, 0, AO_PL | AO_RC}, "p, ground a rectangle");
static_assert(ao_select(4, 20, 0, 10, 2, 1, false, false, true) == AoChoice{4, 0, AO_PL | AO_RC}, "rectangles: never cached");
static_assert(ao_select(3, 20, 0, 10, 1, 1, true, false, false) == AoChoice{0, 0, AO_PL | AO_RC | AO_CNT}, "rectangles, counters");
static_assert(ao_select(16, 20, 0, 10, 1, 1, false, true, false) == AoChoice{16, 0, AO_PL | AO_RC | AO_MF}, "rectangles, multi-frame");
static_assert(ao_select(64, 20, 8, 200, 2, 2, false, false, false) == AoChoice{0, 0, AO_PL | AO_RC | AO_WIDE}, "rectangles, wide");
static_assert(ao_select(16, 20, 8, 64, 0, 0, false, false, true) == ao_select(16, 20, 8, 64, 0, false, false, true), "no rectangle");
static_assert(ao_select(16, 20, 9, 65, 1, 0, false, false, false) == ao_select(16, 20, 9, 65, 1, false, false, false), "planes only");

bool ao_takes_pool_list(const FrameParams& p) {
  return p.mf_n == 0 && (long long)p.trace_rows * p.W < (1ll << 31) &&
         ao_sorts_by_frame(ao_select(p.spp, p.D, p.ncl, p.nobj, p.nplanes, p.nrects, p.counters || p.row_counters, false, true).flags);
}

// Launch ao_batch_kernel<C> over `pools` pools: the LDS rows after the layout hold the sphere
// table (C::PTW: one 64-sphere word of pre-test rows).  A pool-list launch (q.cull_frames == 2):
// over the list's blocks.
template <class C>
inline void launch_ao(long long pools, hipStream_t stream, const FrameParams& q) {
  if (q.cull_frames == 2) pools = ao_pool_list_blocks(q.pool_rot, pools - q.pool_rot);
  const dim3 g((unsigned)pools, C::MF ? (unsigned)q.mf_n : 1u);
  hipLaunchKernelGGL((ao_batch_kernel<C>), g, dim3(64), (size_t)batch_lds<C>(q.spp, C::PTW ? 64 : q.nobj).total, stream,
                     q, q.sph, q.cull);
}
// The production form AoProd<SPPC, DC, FLAGS>, with its launch-log entry
template <int SPPC, int DC, unsigned FLAGS>
inline bool launch_ao_prod(long long pools, hipStream_t stream, const FrameParams& q, LaunchLog* log) {
  if (log) note_launch(log, "ao_batch_kernel<AoProd<%d, %d, %uu>>", SPPC, DC, FLAGS);
  launch_ao<AoProd<SPPC, DC, FLAGS>>(pools, stream, q);
  return true;
}
// An all-sphere scene above kTailMaxObj spheres (AO_WIDE) has at least kB1SortMinObj, so a build
// with the sort selects AO_SORT for it: the unsorted all-sphere shapes have no AO_WIDE forms there.
// (RT_B1_SORT=0, make b1sort0, selects the unsorted ones for every scene and compiles them.)
constexpr bool ao_shape_has_wide(unsigned shape) {
  return (shape & (AO_PL | AO_SORT)) != 0 || !RT_B1_SORT || kB1SortMinObj > kTailMaxObj + 1;
}
// AoChoice -> AoProd.  The library holds exactly the configurations ao_select can return for a
// scene the host can upload: tests/test_kernel_census_cpu.py compares the library's ao_batch_kernel
// symbols with a sweep of the selector (rt_ao_form_host) and fails on a kernel no launch can reach.
// Returns false, launching nothing, for flags that no form was compiled for.
template <int SPPC, int DC, unsigned SHAPE>  // SHAPE: the choice's AO_PL | AO_CLON | AO_SORT | AO_CULLC
inline bool launch_ao_forms(unsigned flags, long long pools, hipStream_t stream, const FrameParams& q, LaunchLog* log) {
  if constexpr (ao_shape_has_wide(SHAPE)) {
    switch (flags & (AO_WIDE | AO_CNT | AO_MF)) {
      case AO_WIDE: return launch_ao_prod<SPPC, DC, SHAPE | AO_WIDE>(pools, stream, q, log);
      case AO_WIDE | AO_CNT: return launch_ao_prod<SPPC, DC, SHAPE | AO_WIDE | AO_CNT>(pools, stream, q, log);
      case AO_WIDE | AO_MF: return launch_ao_prod<SPPC, DC, SHAPE | AO_WIDE | AO_MF>(pools, stream, q, log);
    }
  }
  switch (flags & (AO_WIDE | AO_CNT | AO_MF)) {
    case 0: return launch_ao_prod<SPPC, DC, SHAPE>(pools, stream, q, log);
    case AO_CNT: return launch_ao_prod<SPPC, DC, SHAPE | AO_CNT>(pools, stream, q, log);
    case AO_MF: return launch_ao_prod<SPPC, DC, SHAPE | AO_MF>(pools, stream, q, log);
  }
  return false;
}
template <int SPPC, int DC, unsigned SHAPE>  // SHAPE: the choice's AO_PL | AO_CLON | AO_SORT
inline bool launch_ao_shape(unsigned flags, long long pools, hipStream_t stream, const FrameParams& q, LaunchLog* log) {
  if constexpr (!(SHAPE & AO_PL)) {
    if (flags & AO_CULLC) return launch_ao_forms<SPPC, DC, SHAPE | AO_CULLC>(flags, pools, stream, q, log);
  }
  return launch_ao_forms<SPPC, DC, SHAPE>(flags, pools, stream, q, log);
}
template <unsigned SORT>  // 0 or AO_SORT
inline bool launch_ao_choice(const AoChoice& c, long long pools, hipStream_t stream, const FrameParams& q, LaunchLog* log) {
  if (c.flags & AO_RC) {  // (with AO_PL)
    if constexpr (SORT == 0) {
      if (c.sppc == 16) return launch_ao_shape<16, 0, AO_PL | AO_RC>(c.flags, pools, stream, q, log);
      else if (c.sppc == 4) return launch_ao_shape<4, 0, AO_PL | AO_RC>(c.flags, pools, stream, q, log);
      else return launch_ao_shape<0, 0, AO_PL | AO_RC>(c.flags, pools, stream, q, log);
    }
  } else if (c.flags & AO_PL) {
    if constexpr (SORT == 0) {
      if (c.sppc == 16) return launch_ao_shape<16, 0, AO_PL>(c.flags, pools, stream, q, log);
      else if (c.sppc == 4) return launch_ao_shape<4, 0, AO_PL>(c.flags, pools, stream, q, log);
      else return launch_ao_shape<0, 0, AO_PL>(c.flags, pools, stream, q, log);
    }
  } else if (c.flags & AO_CLON) {
    if (c.sppc == 16) return launch_ao_shape<16, kRefDepth, AO_CLON | SORT>(c.flags, pools, stream, q, log);
    else return launch_ao_shape<64, kRefDepth, AO_CLON | SORT>(c.flags, pools, stream, q, log);
  } else {
    if (c.sppc == 16) return launch_ao_shape<16, 0, SORT>(c.flags, pools, stream, q, log);
    else if (c.sppc == 64) return launch_ao_shape<64, 0, SORT>(c.flags, pools, stream, q, log);
    else if (c.sppc == 4) return launch_ao_shape<4, 0, SORT>(c.flags, pools, stream, q, log);
    else return launch_ao_shape<0, 0, SORT>(c.flags, pools, stream, q, log);
  }
  return false;
}

}  // namespace rt

// The selector as a host entry point (include/rt/abi.h "Kernel forms"): ao_select itself, for the
// census tests.  Touches no GPU.
extern "C" int rt_ao_form_host(int spp, int D, int ncl, int nobj, int nplanes, int nrects, int counters, int multi_frame,
                               int cull_table, int out[3]) {
  if (!out) return RT_E_INVAL;
  const rt::AoChoice c = rt::ao_select(spp, D, ncl, nobj, nplanes, nrects, counters != 0, multi_frame != 0, cull_table != 0);
  out[0] = c.sppc;
  out[1] = c.dc;
  out[2] = (int)c.flags;
  return RT_OK;
}

namespace rt {

// g-buffer layout conversion (rt_download / rt_upload_gbuffer, the host-buffer path of
// compute_one_shader / compute_two_shaders): one thread per reference vec4, reference side
// coalesced.
__global__ __launch_bounds__(256) void gbuf_convert_kernel(GbufXfer x) {
  const size_t total = (size_t)x.F * x.W * x.R;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t wr = (size_t)x.W * x.R;
  const int f = (int)(idx / wr);
  const size_t rem = idx - (size_t)f * wr;
  const int xx = (int)(rem / x.R), r = (int)(rem - (size_t)xx * x.R);
  const size_t o = (size_t)(x.r0 + r) * x.W + xx;
  float4* base = x.slot[f];
  if (x.to_ref) {
    x.ref[idx] = x.kind == 0 ? base[o] : x.kind == 1 ? nrm_load(base, x.n, o) : dep_load(base, x.n, o);
  } else {
    const float4 v = x.ref[idx];
    if (x.kind == 0) base[o] = v;
    else if (x.kind == 1) nrm_store(base, x.n, o, v);
    else dep_store(base, x.n, o, v);
  }
}

hipError_t launch_gbuf_convert(const GbufXfer& x, hipStream_t stream, LaunchLog* log) {
  const size_t total = (size_t)x.F * x.W * x.R;
  if (total == 0) return hipSuccess;
  RT_LAUNCH(log, "gbuf_convert_kernel", gbuf_convert_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x);
  return hipGetLastError();
}

// The blit into the 8-bit framebuffer (src/main.cpp:783-797, shader_fragment.glsl:9-19: colour
// unchanged, alpha 1), rt_quantize_rgba8's rule on the device: NaN and v <= 0 give 0, v >= 1 gives
// 255, else v * 255 + 0.5 in binary32 (two roundings, -ffp-contract=off) truncated; bytes r, g, b,
// 255.  A streaming kernel: 16 B read and 4 B written per pixel, nothing reused.
// As selects, not branches (twelve channels per lane would be twelve exec-mask regions): the value
// converted is always in [0, 255.5), so the cast is defined for every input.
__device__ __forceinline__ unsigned present_channel(float v) {
  const float t = v * 255.0f + 0.5f;
  const float inside = v > 0.0f ? t : 0.0f;  // NaN fails both comparisons: 0
  return (unsigned)(v >= 1.0f ? 255.0f : inside);
}
__device__ __forceinline__ unsigned present_pixel(const float4 v) {
  return present_channel(v.x) | (present_channel(v.y) << 8) | (present_channel(v.z) << 16) | 0xff000000u;
}
// Output row j is image row j, or row rows - 1 - j when top_down.  wide (W % 4 == 0 and `out` 16-byte
// aligned, so every output row is): a lane takes four consecutive pixels of a row, four 16-byte
// loads and one 16-byte store; else one pixel and one 4-byte store per lane (a dword store costs
// several times a dwordx4 store's time per byte: the wide form is the one every frame size in use
// takes).  Blocks of 256 lanes along a row, grid.y over the rows.
__global__ __launch_bounds__(256) void present_kernel(const float4* __restrict__ image, unsigned* __restrict__ out,
                                                      int W, int rows, int top_down, int wide) {
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);  // the lane's unit within a row
  if (u >= (wide ? W >> 2 : W)) return;
  for (int j = (int)blockIdx.y; j < rows; j += (int)gridDim.y) {
    const float4* src = image + (size_t)(top_down ? rows - 1 - j : j) * W;
    unsigned* dst = out + (size_t)j * W;
    if (wide) {
      const float4 a = src[4 * u], b = src[4 * u + 1], c = src[4 * u + 2], d = src[4 * u + 3];
      *(uint4*)(dst + 4 * u) = make_uint4(present_pixel(a), present_pixel(b), present_pixel(c), present_pixel(d));
    } else {
      dst[u] = present_pixel(src[u]);
    }
  }
}

hipError_t launch_present(const float4* image, void* out, int W, int rows, int top_down, hipStream_t stream, LaunchLog* log) {
  if (W <= 0 || rows <= 0) return hipSuccess;
  const int wide = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const int units = wide ? W / 4 : W;
  RT_LAUNCH(log, "present_kernel", present_kernel, dim3((unsigned)((units + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535)),
            dim3(256), 0, stream, image, (unsigned*)out, W, rows, top_down, wide);
  return hipGetLastError();
}

// The blit at window size (rt_present_scaled; the rule is stated in include/rt/abi.h and specified
// by rt_resample_rgba8, rt_host.cpp): the image sampled as the reference's texture is, GL_LINEAR
// with GL_CLAMP_TO_EDGE (src/main.cpp:381-388), then present_channel's conversion.
// One axis: output sample i of `dst` over `src` texels -> the two clamped taps and the weight of
// the second.  n + d > 0, so floor(n / d) is one unsigned division; rem and d are exact in
// binary32 (< 2^16) and the build's '/' is the IEEE division (RT_MATH_DIV).
struct ScaleTap {
  int i0, i1;
  float w;
};
__device__ __forceinline__ ScaleTap scale_tap(int i, int src, int dst) {
  const int n = (2 * i + 1) * src - dst, d = 2 * dst;
  const int x0 = (int)((unsigned)(n + d) / (unsigned)d) - 1;
  const int rem = n - x0 * d;
  return ScaleTap{min(max(x0, 0), src - 1), min(max(x0 + 1, 0), src - 1), (float)rem / (float)d};
}
// (w == 0) ? t0 : (1 - w) * t0 + w * t1 as a select: a zero-weight tap (NaN, inf) never reaches the
// result, and at equal sizes the blit is present_kernel's bit for bit.  u = 1.0f - w, hoisted.
__device__ __forceinline__ float scale_mix(float w, float u, float t0, float t1) {
  const float m = u * t0 + w * t1;
  return w == 0.0f ? t0 : m;
}
__device__ __forceinline__ unsigned scaled_channel(float a, float ua, float b, float ub, float t00, float t01,
                                                   float t10, float t11) {
  return present_channel(scale_mix(b, ub, scale_mix(a, ua, t00, t01), scale_mix(a, ua, t10, t11)));
}
// A lane's N consecutive output pixels of every row it walks.  The column taps are computed once,
// before the row loop (one integer and one float division per column); a row's taps depend on the
// row index alone, so they are wave-uniform.  Per pixel four 16-byte taps at clamped indices:
// nothing outside [R][W] is read.  tx[] is indexed by unrolled constants only (registers).
template <int N>
__device__ __forceinline__ void present_scaled_rows(const float4* __restrict__ image, int W, int R,
                                                    unsigned* __restrict__ out, int out_w, int out_h, int top_down,
                                                    int u) {
  ScaleTap tx[N];
  float ux[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    tx[k] = scale_tap(N * u + k, W, out_w);
    ux[k] = 1.0f - tx[k].w;
  }
  for (int j = (int)blockIdx.y; j < out_h; j += (int)gridDim.y) {
    const ScaleTap ty = scale_tap(top_down ? out_h - 1 - j : j, R, out_h);
    const float uy = 1.0f - ty.w;
    const float4* r0 = image + (size_t)ty.i0 * W;
    const float4* r1 = image + (size_t)ty.i1 * W;
    unsigned px[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float4 p00 = r0[tx[k].i0], p01 = r0[tx[k].i1], p10 = r1[tx[k].i0], p11 = r1[tx[k].i1];
      const float a = tx[k].w, ua = ux[k];
      px[k] = scaled_channel(a, ua, ty.w, uy, p00.x, p01.x, p10.x, p11.x) |
              (scaled_channel(a, ua, ty.w, uy, p00.y, p01.y, p10.y, p11.y) << 8) |
              (scaled_channel(a, ua, ty.w, uy, p00.z, p01.z, p10.z, p11.z) << 16) | 0xff000000u;
    }
    unsigned* dst = out + (size_t)j * out_w + N * u;
    if constexpr (N == 4) *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]);
    else *dst = px[0];
  }
}
// present_kernel's outline: wide (out_w % 4 == 0 and `out` 16-byte aligned) a lane owns four
// consecutive output pixels of a row and writes one 16-byte store, else one pixel and one 4-byte
// store.  Blocks of 256 lanes along the output row, grid.y striding over the output rows.
__global__ __launch_bounds__(256) void present_scaled_kernel(const float4* __restrict__ image, int W, int R,
                                                             unsigned* __restrict__ out, int out_w, int out_h,
                                                             int top_down, int wide) {
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);  // the lane's unit within an output row
  if (u >= (wide ? out_w >> 2 : out_w)) return;
  if (wide) present_scaled_rows<4>(image, W, R, out, out_w, out_h, top_down, u);
  else present_scaled_rows<1>(image, W, R, out, out_w, out_h, top_down, u);
}

// grid.y: about kScaledBlocks workgroups in all, two per CU, so at display sizes a lane walks
// several rows and its column taps are computed once for all of them; never more rows of blocks
// than output rows.  Measured at 512 / 1024 / 2048 / 4096 (DESIGN.md §5 "Round 12"): more
// workgroups never helped (the kernel waits on its loads' cache lines, not on occupancy), and 512
// is the fastest at 3840x2160 -> 1920x1080 (0.027 against 0.034 ms at 1024).
#ifndef RT_SCALED_BLOCKS
#define RT_SCALED_BLOCKS 512  // (A/B builds override it)
#endif
constexpr int kScaledBlocks = RT_SCALED_BLOCKS;
constexpr int kScaledMax = 16384;  // RT_PRESENT_SCALED_MAX: the tap arithmetic is 32-bit
hipError_t launch_present_scaled(const float4* image, int W, int R, void* out, int out_w, int out_h, int top_down,
                                 hipStream_t stream, LaunchLog* log) {
  if (!image || !out || W < 1 || R < 1 || out_w < 1 || out_h < 1 || W > kScaledMax || R > kScaledMax ||
      out_w > kScaledMax || out_h > kScaledMax || ((uintptr_t)out & 3))
    return hipErrorInvalidValue;
  const int wide = out_w % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const int units = wide ? out_w / 4 : out_w;
  const int gx = (units + 255) / 256;
  const int per = kScaledBlocks / gx > 0 ? kScaledBlocks / gx : 1;
  const int gy = out_h < per ? out_h : per;
  RT_LAUNCH(log, "present_scaled_kernel", present_scaled_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, image, W, R,
                     (unsigned*)out, out_w, out_h, top_down, wide);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// ray queries — include/rt/abi.h "Ray queries" (rt_trace_rays / rt_trace_pixels / rt_occluded)
// ---------------------------------------------------------------------------------------
// One sphere of a query's closest-hit scan: sphere_eval_ray (p_compute.glsl:77-109) and the scan's
// acceptance `res > thr && (res < t || t < 0)`, every case of the reference kept (thr is a runtime
// value here and 0 the common one, so none of sphere_candidate's shortcuts, which lean on a literal
// threshold, is taken): del == 0 gives -b, two negative roots give -1, and the square root is
// sqrt_rn, equal to sqrtf on every input.  The tail sits behind a wave-uniform branch as in
// sphere_candidate: when some lane's ray meets the sphere it runs on every active lane and
// del >= 0 joins the acceptance (a negative or NaN discriminant: -1 / NaN in the reference, which
// the scan never accepts).
__device__ __forceinline__ void query_sphere(f3 pos, f3 dir, float4 g, int i, float thr, float& t, int& ind) {
  const f3 pmc = pos - xyz(g);
  const float b = dot(dir, pmc);
  const float del = fmaf(g.w, g.w, fmaf(b, b, -dot(pmc, pmc)));
  const bool meets = del >= 0.0f;
  if (__builtin_amdgcn_ballot_w64(meets) != 0) {
    const float s = sqrt_rn(del);
    const float nb = -1.0f * b;
    const float t1 = nb + s, t2 = nb - s;
    float res = (t2 < 0.0f) ? ((t1 < 0.0f) ? -1.0f : t1) : t2;
    res = (del == 0.0f) ? nb : res;
    const bool acc = meets & (res > thr) & ((res < t) | (t < 0.0f));  // no short-circuit branches
    t = acc ? res : t;
    ind = acc ? i : ind;
  }
}

// The closest-hit scan of a query ray, ascending index (the lowest index wins a tie).  PL = false:
// no plane among the scene's shapes, so the sphere table is scanned (NaN rows for every other
// shape: never accepted).  PL: eval_ray's dispatch on the shape id (p_compute.glsl:121-138), in
// index order, so the scan's own tie rule holds between spheres and planes.  The shape index is
// wave-uniform: the rows come through scalar loads and the id dispatch is a scalar branch.
template <bool PL>
__device__ __forceinline__ int query_closest(const QueryScene& sc, f3 pos, f3 dir, float thr, float& t_out) {
  const float4* __restrict__ geo = sc.shapes;
  const float4* __restrict__ geo2 = sc.shapes + sc.S;
  const float4* __restrict__ sph = sc.shapes + sphere_table(sc.S);
  float t = -1.0f;
  int ind = -1;
  int i = 0;
  if (!PL)  // four rows per scalar load, the same ascending order (the next four are not requested ahead
            // as closest_hit_pf does: each group waits for its load, hidden only by the other waves)
    for (; i + 4 <= sc.nobj; i += 4) {
      const float4 g0 = sph[i], g1 = sph[i + 1], g2 = sph[i + 2], g3 = sph[i + 3];
      query_sphere(pos, dir, g0, i, thr, t, ind);
      query_sphere(pos, dir, g1, i + 1, thr, t, ind);
      query_sphere(pos, dir, g2, i + 2, thr, t, ind);
      query_sphere(pos, dir, g3, i + 3, thr, t, ind);
    }
  for (; i < sc.nobj; ++i) {
    if (!PL) {
      query_sphere(pos, dir, sph[i], i, thr, t, ind);
    } else {
      const float4 g = geo[i], g2 = geo2[i];
      const int id = __float_as_int(g2.w);
      if (id == SHAPE_SPHERE) {
        query_sphere(pos, dir, g, i, thr, t, ind);
      } else if (id == SHAPE_PLANE) {
        const float res = plane_eval(pos, dir, g, g2);
        const bool acc = (res > thr) & ((res < t) | (t < 0.0f));
        t = acc ? res : t;
        ind = acc ? i : ind;
      }
    }
  }
  t_out = t;
  return ind;
}

// One ray per lane.  PIX: the camera's ray through pixel xy[i], formed as the frame kernels form it
// (primary_dir on x / W and y / H; the division is the IEEE one, whose value div_rn_by returns for
// the frame kernels' in-frame coordinates, because a query's coordinates may be any int32).
template <bool PL, bool PIX>
__global__ __launch_bounds__(kBlock) void ray_query_kernel(RayQuery Q) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= Q.n) return;
  f3 o, d;
  if (PIX) {
    const int x = Q.xy[2 * i], y = Q.xy[2 * i + 1];
    o = mk(Q.sc.cx, Q.sc.cy, Q.sc.cz);
    d = primary_dir(Q.sc, (float)x / Q.sc.fW, (float)y / Q.sc.fH);
  } else {
    o = mk(Q.origins[3 * i], Q.origins[3 * i + 1], Q.origins[3 * i + 2]);
    d = mk(Q.dirs[3 * i], Q.dirs[3 * i + 1], Q.dirs[3 * i + 2]);
  }
  float t;
  const int ind = query_closest<PL>(Q.sc, o, d, Q.thr, t);
  if (Q.t) Q.t[i] = t;
  if (Q.ind) Q.ind[i] = ind;
  if (Q.nrm) {
    f3 n = mk(0.0f, 0.0f, 0.0f);
    if (ind >= 0) {  // the Phong g-buffer's normal (phong_tile): of shape ind at o + t * d
      const int id = PL ? __float_as_int(Q.sc.shapes[Q.sc.S + ind].w) : SHAPE_SPHERE;
      n = shape_normal(Q.sc.shapes[ind], id, o + t * d);
    }
    Q.nrm[3 * i] = n.x;
    Q.nrm[3 * i + 1] = n.y;
    Q.nrm[3 * i + 2] = n.z;
  }
  if (PIX && Q.dir_out) {
    Q.dir_out[3 * i] = d.x;
    Q.dir_out[3 * i + 1] = d.y;
    Q.dir_out[3 * i + 2] = d.z;
  }
}

// One segment per lane: shadow_ray (p_compute.glsl:145-166) from from[i] towards to[i]; out = !lit.
template <bool PL>
__global__ __launch_bounds__(kBlock) void occluded_kernel(QueryScene sc, const float* __restrict__ from,
                                                          const float* __restrict__ to, size_t n,
                                                          unsigned char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 a = mk(from[3 * i], from[3 * i + 1], from[3 * i + 2]);
  const f3 b = mk(to[3 * i], to[3 * i + 1], to[3 * i + 2]);
  const bool lit = PL ? shadow_lit<false>(sc.shapes, sc.shapes + sc.S, sc.nobj, b, a)
                      : shadow_lit<true>(sc.shapes + sphere_table(sc.S), nullptr, sc.nobj, b, a);
  out[i] = lit ? 0 : 1;
}

// Rectangles in effect (sc.nrects > 0; include/rt/abi.h "Rectangles"): the spheres over the sphere
// table (query_closest<false>'s scan), then every entry of the plane table, planes and rectangles,
// merged by planar_candidate's (t, index) rule: the result of eval_ray's ascending scan whatever the
// visiting order, as in the frame kernels.
__device__ __forceinline__ int query_closest_rc(const QueryScene& sc, f3 pos, f3 dir, float thr, float& t_out) {
  float t;
  int ind = query_closest<false>(sc, pos, dir, thr, t);
  const float4* __restrict__ planes = sc.shapes + plane_table(sc.S);
  for (int k = 0; k < sc.nplanes; ++k)
    planar_candidate<true>(planes, pos, dir, planes[2 * k], planes[2 * k + 1], thr, t, ind);
  t_out = t;
  return ind;
}

// ray_query_kernel<true, PIX> over a plane table with rectangles in effect; an entry point of its own,
// so the kernels above keep their names and code.
template <bool PIX>
__global__ __launch_bounds__(kBlock) void ray_query_rc_kernel(RayQuery Q) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= Q.n) return;
  f3 o, d;
  if (PIX) {
    const int x = Q.xy[2 * i], y = Q.xy[2 * i + 1];
    o = mk(Q.sc.cx, Q.sc.cy, Q.sc.cz);
    d = primary_dir(Q.sc, (float)x / Q.sc.fW, (float)y / Q.sc.fH);
  } else {
    o = mk(Q.origins[3 * i], Q.origins[3 * i + 1], Q.origins[3 * i + 2]);
    d = mk(Q.dirs[3 * i], Q.dirs[3 * i + 1], Q.dirs[3 * i + 2]);
  }
  float t;
  const int ind = query_closest_rc(Q.sc, o, d, Q.thr, t);
  if (Q.t) Q.t[i] = t;
  if (Q.ind) Q.ind[i] = ind;
  if (Q.nrm) {
    f3 n = mk(0.0f, 0.0f, 0.0f);
    if (ind >= 0) n = shape_normal_rc<true>(Q.sc.shapes[ind], __float_as_int(Q.sc.shapes[Q.sc.S + ind].w), o + t * d);
    Q.nrm[3 * i] = n.x;
    Q.nrm[3 * i + 1] = n.y;
    Q.nrm[3 * i + 2] = n.z;
  }
  if (PIX && Q.dir_out) {
    Q.dir_out[3 * i] = d.x;
    Q.dir_out[3 * i + 1] = d.y;
    Q.dir_out[3 * i + 2] = d.z;
  }
}

// occluded_kernel<true> over a plane table with rectangles in effect: shadow_ray with the plane
// table's entries first, then the sphere table ("some occluder exists" does not depend on the order).
__global__ __launch_bounds__(kBlock) void occluded_rc_kernel(QueryScene sc, const float* __restrict__ from,
                                                             const float* __restrict__ to, size_t n,
                                                             unsigned char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 pos = mk(from[3 * i], from[3 * i + 1], from[3 * i + 2]);
  const f3 lv = mk(to[3 * i], to[3 * i + 1], to[3 * i + 2]) - pos;
  const f3 l = normalize(lv);
  const float len = sqrtf(dot(lv, lv));
  const f3 np = pos + 0.01f * l;
  const double dlen = (double)len;
  const float4* __restrict__ planes = sc.shapes + plane_table(sc.S);
  const float4* __restrict__ sph = sc.shapes + sphere_table(sc.S);
  bool occ = false;
  for (int k = 0; k < sc.nplanes && !occ; ++k)
    occ = shadow_occludes(planar_eval<true>(planes, np, l, planes[2 * k], planes[2 * k + 1]), l, dlen);
  for (int k = 0; k < sc.nobj && !occ; ++k) occ = shadow_occludes(sphere_eval_shadow(np, l, sph[k]), l, dlen);
  out[i] = occ ? 1 : 0;
}

// ---------------------------------------------------------------------------------------
// The query tree (include/rt/abi.h "Query tree"; rt_plan build_query_tree): the queries above over
// a tree of balls around the spheres, the same answers bit for bit.
// ---------------------------------------------------------------------------------------
// The closest hit of a ray over the tree: the always list (wave-uniform entries: scalar loads), the
// tree, each lane walking the preorder array with its own index (vector loads: the lanes diverge),
// then every entry of the plane table as query_closest_rc scans it (a plane's entry has offset 0, so
// planar_candidate<true> is plane_candidate on it; plane_eval on the plane table's rows is plane_eval
// on geo / geo2: the same normal and p0).  No stack: a node whose ball may be hit is followed by its
// first child or, for a leaf, by its members and then the next node; any other by its skip link.
// A culled ball's members are never accepted by the linear scan (cluster_may_hit's cases (A) and
// (B): a computed del < 0, or both roots negative, which no thr >= 0 accepts), and the merge does not
// depend on the order, so (t, ind) are the linear scan's.  Nothing is pruned by the current t.
__device__ __forceinline__ int tree_closest(const QueryScene& sc, const QueryTree& T, f3 pos, f3 dir, float thr,
                                            float& t_out) {
  float t = -1.0f;
  int ind = -1;
  const float4* __restrict__ rows = T.rows;
  const int* __restrict__ index = T.index;
  for (int e = T.always_first; e < T.always_first + T.n_always; ++e) tree_sphere(pos, dir, rows[e], index[e], thr, t, ind);
  const bool gate = unit_gate(dir);
  const float4* __restrict__ nodes = T.nodes;
  for (int k = 0; k < T.n_nodes;) {
    const float4 cb = nodes[2 * k], lk = nodes[2 * k + 1];
    if (tree_may_hit(gate, pos, dir, cb)) {
      const int first = __float_as_int(lk.y), count = __float_as_int(lk.z);
      for (int j = 0; j < count; ++j) tree_sphere(pos, dir, rows[first + j], index[first + j], thr, t, ind);
      k = k + 1;
    } else {
      k = __float_as_int(lk.x);
    }
  }
  const float4* __restrict__ planes = sc.shapes + plane_table(sc.S);
  for (int k = 0; k < sc.nplanes; ++k)
    planar_candidate<true>(planes, pos, dir, planes[2 * k], planes[2 * k + 1], thr, t, ind);
  t_out = t;
  return ind;
}

// ray_query_rc_kernel over the tree: the rays, normals and dir_out formed exactly as there
// (shape_normal_rc<true> is shape_normal on a sphere or a plane, and only a rectangle in effect is hit).
template <bool PIX>
__global__ __launch_bounds__(kBlock) void ray_query_tree_kernel(RayQuery Q, QueryTree T) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= Q.n) return;
  f3 o, d;
  if (PIX) {
    const int x = Q.xy[2 * i], y = Q.xy[2 * i + 1];
    o = mk(Q.sc.cx, Q.sc.cy, Q.sc.cz);
    d = primary_dir(Q.sc, (float)x / Q.sc.fW, (float)y / Q.sc.fH);
  } else {
    o = mk(Q.origins[3 * i], Q.origins[3 * i + 1], Q.origins[3 * i + 2]);
    d = mk(Q.dirs[3 * i], Q.dirs[3 * i + 1], Q.dirs[3 * i + 2]);
  }
  float t;
  const int ind = tree_closest(Q.sc, T, o, d, Q.thr, t);
  if (Q.t) Q.t[i] = t;
  if (Q.ind) Q.ind[i] = ind;
  if (Q.nrm) {
    f3 n = mk(0.0f, 0.0f, 0.0f);
    if (ind >= 0) n = shape_normal_rc<true>(Q.sc.shapes[ind], __float_as_int(Q.sc.shapes[Q.sc.S + ind].w), o + t * d);
    Q.nrm[3 * i] = n.x;
    Q.nrm[3 * i + 1] = n.y;
    Q.nrm[3 * i + 2] = n.z;
  }
  if (PIX && Q.dir_out) {
    Q.dir_out[3 * i] = d.x;
    Q.dir_out[3 * i + 1] = d.y;
    Q.dir_out[3 * i + 2] = d.z;
  }
}

// occluded_rc_kernel over the tree: shadow_ray's set-up as there, the plane table first, then the
// always list, then the tree with the ray (np, l); out on the first occluder.  A culled ball's
// members are spheres for which sphere_eval_shadow returns what shadow_occludes rejects:
// sphere_eval_shadow forms pmc, b and del with the float operations of query_sphere (the ones the
// proof's error bounds are about), returns -1 for a computed del < 0 (case (A)), and in case (B),
// both roots negative by more than ten times their error, -1 again whichever of sqrt_rn_tail's
// roots is taken (equal to sqrtf's above 2^-96, at most 2^-47 below); -1 > 0.0001 is false.
__global__ __launch_bounds__(kBlock) void occluded_tree_kernel(QueryScene sc, QueryTree T, const float* __restrict__ from,
                                                               const float* __restrict__ to, size_t n,
                                                               unsigned char* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 pos = mk(from[3 * i], from[3 * i + 1], from[3 * i + 2]);
  const f3 lv = mk(to[3 * i], to[3 * i + 1], to[3 * i + 2]) - pos;
  const f3 l = normalize(lv);
  const float len = sqrtf(dot(lv, lv));
  const f3 np = pos + 0.01f * l;
  const double dlen = (double)len;
  const float4* __restrict__ planes = sc.shapes + plane_table(sc.S);
  const float4* __restrict__ rows = T.rows;
  bool occ = false;
  for (int k = 0; k < sc.nplanes && !occ; ++k)
    occ = shadow_occludes(planar_eval<true>(planes, np, l, planes[2 * k], planes[2 * k + 1]), l, dlen);
  for (int e = T.always_first; e < T.always_first + T.n_always && !occ; ++e)
    occ = shadow_occludes(sphere_eval_shadow(np, l, rows[e]), l, dlen);
  const bool gate = unit_gate(l);
  const float4* __restrict__ nodes = T.nodes;
  for (int k = 0; k < T.n_nodes && !occ;) {
    const float4 cb = nodes[2 * k], lk = nodes[2 * k + 1];
    if (tree_may_hit(gate, np, l, cb)) {
      const int first = __float_as_int(lk.y), count = __float_as_int(lk.z);
      for (int j = 0; j < count && !occ; ++j) occ = shadow_occludes(sphere_eval_shadow(np, l, rows[first + j]), l, dlen);
      k = k + 1;
    } else {
      k = __float_as_int(lk.x);
    }
  }
  out[i] = occ ? 1 : 0;
}

constexpr size_t kQueryMaxRays = (size_t)1 << 28;  // RT_QUERY_MAX_RAYS: the grid's x stays below 2^31

static bool has_tree(const QueryTree* tree) {
  return tree && tree->n_nodes > 0 && tree->nodes && tree->rows && tree->index;
}

hipError_t launch_ray_query(const RayQuery& q, hipStream_t stream, const QueryTree* tree, LaunchLog* log) {
  if (q.n == 0) return hipSuccess;
  if (q.n > kQueryMaxRays || !q.sc.shapes || (!q.xy && (!q.origins || !q.dirs))) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((q.n + kBlock - 1) / kBlock));
  if (has_tree(tree)) {
    if (q.xy) RT_LAUNCH(log, "ray_query_tree_kernel<true>", ray_query_tree_kernel<true>, grid, dim3(kBlock), 0, stream, q, *tree);
    else RT_LAUNCH(log, "ray_query_tree_kernel<false>", ray_query_tree_kernel<false>, grid, dim3(kBlock), 0, stream, q, *tree);
    return hipGetLastError();
  }
  const bool pl = q.sc.nplanes > 0;
  if (pl && q.sc.nrects > 0) {  // rectangles in effect: the RC twins
    if (q.xy) RT_LAUNCH(log, "ray_query_rc_kernel<true>", ray_query_rc_kernel<true>, grid, dim3(kBlock), 0, stream, q);
    else RT_LAUNCH(log, "ray_query_rc_kernel<false>", ray_query_rc_kernel<false>, grid, dim3(kBlock), 0, stream, q);
    return hipGetLastError();
  }
  if (q.xy) {
    if (pl) RT_LAUNCH(log, "ray_query_kernel<true, true>", (ray_query_kernel<true, true>), grid, dim3(kBlock), 0, stream, q);
    else RT_LAUNCH(log, "ray_query_kernel<false, true>", (ray_query_kernel<false, true>), grid, dim3(kBlock), 0, stream, q);
  } else {
    if (pl) RT_LAUNCH(log, "ray_query_kernel<true, false>", (ray_query_kernel<true, false>), grid, dim3(kBlock), 0, stream, q);
    else RT_LAUNCH(log, "ray_query_kernel<false, false>", (ray_query_kernel<false, false>), grid, dim3(kBlock), 0, stream, q);
  }
  return hipGetLastError();
}

hipError_t launch_occluded(const QueryScene& sc, const float* from, const float* to, size_t n, unsigned char* out,
                           hipStream_t stream, const QueryTree* tree, LaunchLog* log) {
  if (n == 0) return hipSuccess;
  if (n > kQueryMaxRays || !sc.shapes || !from || !to || !out) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (has_tree(tree)) RT_LAUNCH(log, "occluded_tree_kernel", occluded_tree_kernel, grid, dim3(kBlock), 0, stream, sc, *tree, from, to, n, out);
  else if (sc.nplanes > 0 && sc.nrects > 0) RT_LAUNCH(log, "occluded_rc_kernel", occluded_rc_kernel, grid, dim3(kBlock), 0, stream, sc, from, to, n, out);
  else if (sc.nplanes > 0) RT_LAUNCH(log, "occluded_kernel<true>", occluded_kernel<true>, grid, dim3(kBlock), 0, stream, sc, from, to, n, out);
  else RT_LAUNCH(log, "occluded_kernel<false>", occluded_kernel<false>, grid, dim3(kBlock), 0, stream, sc, from, to, n, out);
  return hipGetLastError();
}

// The production launch of `program` (rt_kernels.hip's launch_program; the A/B tools library
// falls back to it): q = p with the derived table pointers and launch constants.
inline FrameParams launch_params(const FrameParams& p) {
  FrameParams q = p;
  q.sph = p.shapes + sphere_table(p.S);
  q.planes = p.shapes + plane_table(p.S);
  q.clus = p.shapes + cluster_table(p.S);
  q.clmask = (const unsigned long long*)(p.shapes + cluster_mask_table(p.S));
  q.camrel = p.shapes + camrel_table(p.S);
  q.b1_min = 1;
  {  // rotation group: the pools of one image row (at least 8)
    const int TP = kPool / p.spp > 0 ? kPool / p.spp : 1;
    const int ppr = p.W / TP;
    q.pool_rot = ppr >= 8 ? ppr : 8;
    if (p.cull_frames == 2) q.pool_rot = p.pool_rot;  // a pool-list launch: the list's non-sky pools
  }
  {  // post-process XCD runs (xcd_tile): the least R in [4, gx / 16] dividing gx / 8 (a tile row
    // is a whole number of 8-run rounds, at least two per XCD), else 4; narrow frames: none
    const int gx = (p.W + kPostTileW - 1) / kPostTileW;
    int R = 0;
    if (gx % 8 == 0)
      for (int r = 4; r <= gx / 16 && !R; ++r)
        if ((gx / 8) % r == 0) R = r;
    q.tile_run = R ? R : (gx >= 32 ? 4 : 0);
#ifdef RT_POST_RUN
    q.tile_run = RT_POST_RUN;  // A/B builds: a fixed run length (0 = row-major order)
#endif
    // super-tiles (xcd_tile): 4 or 2 blocks each way where that divides the grid
    const int gy = (p.trace_rows + kPostTileH - 1) / kPostTileH;
    q.post_sx = gx % 4 == 0 ? 4 : (gx % 2 == 0 ? 2 : 1);
    q.post_sy = gy % 4 == 0 ? 4 : (gy % 2 == 0 ? 2 : 1);
    if (gx < 8 * q.post_sx) q.post_sx = q.post_sy = 1;  // narrow frames: the runs (or none)
  }
  return q;
}

inline hipError_t launch_production(int program, const FrameParams& p, const FrameParams& q, hipStream_t stream,
                                    LaunchLog* log = nullptr) {
  const bool pl = p.nplanes > 0;
  if (program == K_AOP || program == K_AO) {
    const long long npix = (long long)p.trace_rows * p.W;
    const int TP = kPool / p.spp > 0 ? kPool / p.spp : 1;
    const long long pools = (npix + TP - 1) / TP;
    const AoChoice c = ao_select(p.spp, p.D, p.ncl, p.nobj, p.nplanes, p.nrects, p.counters || p.row_counters,
                                 p.mf_n > 0, q.cull != nullptr);
    // a pool list only with a form that reads it, and counts that are a split of the pools
    if (q.cull_frames == 2 && (!q.cull || !ao_takes_pool_list(p) || q.pool_rot < 0 || q.pool_rot > pools))
      return hipErrorInvalidValue;
    // (kSortBit: a build with RT_B1_SORT=0 never selects the sort and compiles no SORT instantiation)
    const bool launched = (c.flags & AO_SORT) ? launch_ao_choice<kSortBit>(c, pools, stream, q, log)
                                              : launch_ao_choice<0>(c, pools, stream, q, log);
    return launched ? hipGetLastError() : hipErrorInvalidValue;  // (no compiled form: an error, not a silent skip)
  }
  // modes 3/4 multi-frame launches: FPB frames per block (block_frames)
  const int fpb = program == K_PHONG ? kPhongFramesPerBlock : kHybridFramesPerBlock;
  // hybrid blocks: kHyBW x kHyBW waves of 8x8 pixels (kHyTile = 8 kHyBW px); phong: 2x2 waves
  const int tw = program == K_HYBRID ? kHyTile : 16;
  dim3 grid((p.W + tw - 1) / tw, (p.trace_rows + tw - 1) / tw, p.mf_n > 0 ? (p.mf_n + fpb - 1) / fpb : 1);
  const dim3 hyb(64 * kHyBW * kHyBW);
  // The shape tables are read through the caches (scalar loads for the wave-uniform culls and
  // survivor tests, vector loads for the hit's material), not staged in LDS per block (the LT
  // instantiations, A/B tools library only)
  const bool mf = p.mf_n > 0;  // multi-frame launch; single-frame ones take the MF = false kernels
  if (pl && p.nrects > 0 && (program == K_PHONG || program == K_HYBRID)) {  // rectangles in effect: the RC twins
    const bool gb = p.phong_gbuf != 0;
    if (program == K_PHONG) {
      if (mf && gb) RT_LAUNCH(log, "phong_rc_kernel<true, true>", (phong_rc_kernel<true, true>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (mf) RT_LAUNCH(log, "phong_rc_kernel<true, false>", (phong_rc_kernel<true, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (gb) RT_LAUNCH(log, "phong_rc_kernel<false, true>", (phong_rc_kernel<false, true>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else RT_LAUNCH(log, "phong_rc_kernel<false, false>", (phong_rc_kernel<false, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
    } else {
      if (mf && gb) RT_LAUNCH(log, "hybrid_rc_kernel<" RT_HYBW ", true, true>", (hybrid_rc_kernel<kHyBW, kHyBW, true, true>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (mf) RT_LAUNCH(log, "hybrid_rc_kernel<" RT_HYBW ", true, false>", (hybrid_rc_kernel<kHyBW, kHyBW, true, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (gb) RT_LAUNCH(log, "hybrid_rc_kernel<" RT_HYBW ", false, true>", (hybrid_rc_kernel<kHyBW, kHyBW, false, true>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else RT_LAUNCH(log, "hybrid_rc_kernel<" RT_HYBW ", false, false>", (hybrid_rc_kernel<kHyBW, kHyBW, false, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
    }
    return hipGetLastError();
  }
  if (p.phong_gbuf && (program == K_PHONG || program == K_HYBRID)) {  // rt_set_phong_gbuffer: the GB instantiations
    if (program == K_PHONG) {
      if (pl && mf) RT_LAUNCH(log, "phong_gbuf_kernel<true, true>", (phong_gbuf_kernel<true, true>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (pl) RT_LAUNCH(log, "phong_gbuf_kernel<true, false>", (phong_gbuf_kernel<true, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (mf) RT_LAUNCH(log, "phong_gbuf_kernel<false, true>", (phong_gbuf_kernel<false, true>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else RT_LAUNCH(log, "phong_gbuf_kernel<false, false>", (phong_gbuf_kernel<false, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
    } else {
      if (pl && mf) RT_LAUNCH(log, "hybrid_gbuf_kernel<true, " RT_HYBW ", true>", (hybrid_gbuf_kernel<true, kHyBW, kHyBW, true>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (pl) RT_LAUNCH(log, "hybrid_gbuf_kernel<true, " RT_HYBW ", false>", (hybrid_gbuf_kernel<true, kHyBW, kHyBW, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (mf) RT_LAUNCH(log, "hybrid_gbuf_kernel<false, " RT_HYBW ", true>", (hybrid_gbuf_kernel<false, kHyBW, kHyBW, true>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else RT_LAUNCH(log, "hybrid_gbuf_kernel<false, " RT_HYBW ", false>", (hybrid_gbuf_kernel<false, kHyBW, kHyBW, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
    }
    return hipGetLastError();
  }
  switch (program) {
    case K_PHONG:
      if (pl && mf) RT_LAUNCH(log, "phong_kernel<true, true, false, true>", (phong_kernel<true, true, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (pl) RT_LAUNCH(log, "phong_kernel<true, true, false, false>", (phong_kernel<true, true, false, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else if (mf) RT_LAUNCH(log, "phong_kernel<true, false, false, true>", (phong_kernel<true, false, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      else RT_LAUNCH(log, "phong_kernel<true, false, false, false>", (phong_kernel<true, false, false, false>), grid, dim3(kBlock), 0, stream, q.sph, q.shapes, q);
      break;
    case K_HYBRID:
      if (pl && mf) RT_LAUNCH(log, "hybrid_kernel<true, true, false, 0, " RT_HYBW ", true>", (hybrid_kernel<true, true, false, 0, kHyBW, kHyBW>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (pl) RT_LAUNCH(log, "hybrid_kernel<true, true, false, 0, " RT_HYBW ", false>", (hybrid_kernel<true, true, false, 0, kHyBW, kHyBW, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else if (mf) RT_LAUNCH(log, "hybrid_kernel<true, false, false, 0, " RT_HYBW ", true>", (hybrid_kernel<true, false, false, 0, kHyBW, kHyBW>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      else RT_LAUNCH(log, "hybrid_kernel<true, false, false, 0, " RT_HYBW ", false>", (hybrid_kernel<true, false, false, 0, kHyBW, kHyBW, false>), grid, hyb, 0, stream, q.tile_order, q.sph, q.shapes, grid.x, q);
      break;
    case K_POST:
      RT_LAUNCH(log, "post_kernel", post_kernel,
                         dim3((p.W + kPostTileW - 1) / kPostTileW, (p.trace_rows + kPostTileH - 1) / kPostTileH),
                         dim3(kBlock), 0, stream, q);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_selftest(int fn, const float* d_in, float* d_out, size_t n, hipStream_t stream, LaunchLog* log) {
  if (n == 0) return hipSuccess;
  const size_t lanes = selftest_wave_fn(fn) ? n * 64 : n;
  unsigned grid = (unsigned)((lanes + 255) / 256);
  RT_LAUNCH(log, "selftest_kernel", selftest_kernel, dim3(grid), dim3(256), 0, stream, fn, d_in, d_out, n);
  return hipGetLastError();
}

}  // namespace rt
