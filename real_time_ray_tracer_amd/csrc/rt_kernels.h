// rt_kernels.h — launch interface between the C-ABI shim and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rt_table.h"

// Normals slot layout, shared by the kernels and the shim (rt_download_rect reads the slots
// directly): 1 = an xyz plane then a w plane (production), 0 = interleaved float4 (the round-2
// layout, A/B builds only; set it for both translation units or neither).
#ifndef RT_NRM_PLANES
#define RT_NRM_PLANES 1
#endif

namespace rt {

constexpr int kMaxFrames = 16;
// (kMaxBatch, the frames per multi-frame launch, and the device table layout: rt_table.h)
// Hybrid (mode 4) workgroups of kHyBW x kHyBW waves, each wave an 8x8 pixel tile; the tile
// schedule's units are these workgroups (rt_shim launch_sched).  2x2 (16x16 pixels, 4 waves).
// Round 5 A/Bs at (b), tables read through the caches: in row order 1x1 33.1, 2x1 33.6, 2x2 34.2,
// 4x1 33.7, 4x2 35.0 us per launch (profiles/r05o_*), but with the longest-first schedule 1x1
// (its order at 8x8 granularity) 28.3 vs 2x2 26.5 us (r05p_*).  Set for both translation units.
#ifndef RT_HY_BW
#define RT_HY_BW 2
#endif
constexpr int kHyBW = RT_HY_BW, kHyTile = 8 * RT_HY_BW;
constexpr int kCounters = 8;
constexpr int kCounterSlots = 256;  // per counter, summed by the host

// Everything one program launch needs.  Passed by value as the kernel argument (lives in the
// kernarg segment -> SGPRs).  Row ranges are in frame coordinates (row 0 = bottom row).
struct FrameParams {
  int W, H;                  // full frame (WIDTH, HEIGHT)
  int trace_row0, trace_rows;  // rows this launch computes
  int band_row0, band_rows;  // rows held by the g-buffer ring (strip + halo)
  int img_row0, img_rows;    // rows of the image (the strip, no halo)
  int nobj;                  // int(mode.z)
  int S;                     // stride of the compact shape table (capacity)
  int spp, D, F, frame;
  int b1_min;                // AO: least live lanes of a prepared batch for its batched first bounce (set at launch)
  int pool_rot;              // AO: pools per rotation group (one row's; 0 = pools in row order; set at launch); a pool-list
                             // launch (cull_frames == 2) has no rotation: the list's non-sky pools, set by the cull cache
  int tile_run;              // post-process: tiles per XCD run (xcd_tile; set at launch)
  int post_sx, post_sy;      // post-process: super-tiles of post_sx x post_sy blocks per XCD visit (xcd_tile)
  float inv_spp, fW, fH;     // 1.0f / spp, (float)W, (float)H: host-computed wave-uniform constants
  float inv_W, inv_H;        // 1.0f / fW, 1.0f / fH (correctly rounded; div_rn_by)
  float hx, hy, hz;          // horizontal
  float vx, vy, vz;          // vertical
  float lx, ly, lz;          // llc_minus_campos
  float cx, cy, cz;          // camera_location
  float Lx, Ly, Lz;          // light_pos
  int cull_frames;           // AO: `cull` is preceded by the pools' sort frames (below); in the padding in front of bg,
                             // so no other member and no kernel argument moves
  float4 bg;                 // background
  const float4* shapes;      // compact table [4][S]: geo, geo2, col, aux (rt_device.h)
  // derived from `shapes` by launch_program (sphere_table / plane_table below):
  const float4* sph;         // [S] sphere-only geometry: geo for spheres, NaN for every other shape
  const float4* planes;      // [nplanes][2]: (normal, bits(index)), (p0, 0) of the planes among [0, nobj)
  int nplanes;               // set by the host (rt_shim) from the header's shape ids
  int phong_gbuf;            // modes 3/4: launch the instantiations that also write nrm / dep (rt_set_phong_gbuffer);
                             // read by the launcher only, in the padding behind nplanes, so no other member moves
  // AO bounce-ray cluster culling (set by the host, rt_shim build_clusters; ncl = 0: off):
  const float4* clus;        // [ncl] (centre, R): every member sphere lies within R of the centre
  const unsigned long long* clmask;  // [1 + kMaxClusters][kClusterWords]: always-tested spheres, then members
  const float4* camrel;              // [S] (camera - centre, |camera - centre|^2 as the kernels' dot) per sphere
  int ncl;
  int nrects;                // rectangles in effect among the plane table's nplanes entries (rt_table.h rect_table); read
                             // by the launcher only (> 0: the RC instantiations), in the padding behind ncl, so no
                             // other member moves
  const float4* rb;          // rand_buffer[2*spp]
  float4* out_pix;           // colour destination [band_rows][W]
  float4* nrm;               // normals_buffer slot `frame` [band_rows][W]
  float4* dep;               // depth_buffer slot `frame`
  const float4* nrm_prev;    // the slot's previous normals / depth (stale reads); == nrm / dep
  const float4* dep_prev;    // unless the frame is pipelined (written to a fresh buffer)
  float4* image;             // [img_rows][W] or nullptr
  const float4* raw;         // post-process input (pre-filter snapshot of slot `frame`)
  const float4* hist_pix[kMaxFrames];  // per slot
  const float4* hist_nrm[kMaxFrames];
  const float4* hist_dep[kMaxFrames];
  // optional work counters (nullptr in timed runs): [0] primary samples, [1] closest-hit
  // segments, [2] shadow rays, [3] ray-shape tests = (segments + shadow rays) * nobj,
  // [4] executed lane-tests = sum over waves of 64 x (shapes tested by the wave's scene loops);
  // post-process: [5] filtered pixels, [6] history slots read, [7] history slots accepted;
  // each counter has kCounterSlots copies (index k * kCounterSlots + slot)
  unsigned long long* counters;
  // optional per-row closest-hit segment counts, indexed by (y - band_row0) (nullptr = off)
  unsigned long long* row_counters;
  // multi-frame Phong/hybrid launch (mf_n > 0, gridDim.z = mf_n): frame j of the batch renders
  // into slot (mf_slot0 + j) % F (hist_pix) with light mf_light[j]; only frame mf_n - 1 writes
  // the image.  The shape table is the same for every frame of the batch.
  int mf_n, mf_slot0;
  float4 mf_light[kMaxBatch];
  // multi-frame AO launch (mode 2, gridDim.y = mf_n): frame j reads rand_buffer mf_rb[j * 2 spp ..]
  // and writes slot (mf_slot0 + j) % F (hist_pix / hist_nrm / hist_dep); the image by frame mf_n - 1
  const float4* mf_rb;
  // hybrid (mode 4) tile schedule (rt_sched.h TileSched): block (x, y) renders the 16x16 tile
  // tile_order[x + y * gridDim.x] (packed x | y << 16) when non-null, else tile (x, y); each wave
  // stores its bounce-round count at tile_cost[tile * 4 + wave] when non-null
  const unsigned* tile_order;
  unsigned* tile_cost;
  // AO, all-sphere scenes: the pools' primary-ray cull masks, [pools][(nobj + 63) / 64] u64 as
  // launch_cull_fill wrote them for this camera, scene and strip; non-null selects the kernels
  // that load their pool's masks instead of computing them (nullptr: the in-kernel cull).
  // cull_frames != 0: the same allocation holds, in front of the masks, pool pb's sort frame at
  // (const float4*)cull - 2 (pb + 1): (e1, 0), (e2, 0), two unit vectors orthogonal to the surface
  // normal at the hit of the pool's unjittered centre ray (launch_cull_fill); the sorted kernels
  // then deal the pool's samples by the sector of their bounce hemisphere point around that normal
  // cull_frames == 2 (single-frame launches of those kernels only, ao_takes_pool_list): in front of
  // the frames the allocation holds the pool list as well (ao_pool_list_bytes), and the grid is
  // ao_pool_list_blocks(pool_rot, pools - pool_rot): block b < pool_rot renders the pool of the
  // list's row b, read with one scalar load in place of the pool start's index arithmetic, and
  // each later block stores 64 of the list's sky pools
  const unsigned long long* cull;
};
static_assert(offsetof(FrameParams, bg) == 160 && offsetof(FrameParams, cull_frames) == 156,
              "cull_frames fills the padding in front of bg");
static_assert(offsetof(FrameParams, phong_gbuf) == 204 && offsetof(FrameParams, clus) == 208,
              "phong_gbuf fills the padding behind nplanes");
static_assert(offsetof(FrameParams, ncl) == 232 && offsetof(FrameParams, nrects) == 236 && offsetof(FrameParams, rb) == 240,
              "nrects fills the padding behind ncl");

// bytes of the sort frames in front of a cull table of `pools` pools (two float4 per pool)
constexpr size_t ao_cull_frame_bytes(long long pools) { return (size_t)pools * 2 * sizeof(float4); }

// The pool list, in front of the sort frames in the same allocation (launch_pool_list writes it from
// the masks; FrameParams::cull_frames == 2 selects it).  From its first byte:
//   16 x pools bytes  the non-sky pools' rows upwards from the start, int4 (pb, xf, yf, np) in
//                     ascending pb: a pool with a sphere in its masks, the first pixel's column and
//                     frame row and the pool's pixel count as ao_batch_kernel's pool start forms
//                     them; the sky pools' pb, 4 bytes each, downwards from the end (entry j at
//                     ((unsigned*)end)[-1 - j], ascending too): 16 n_nonsky + 4 n_sky <= 16 pools
//   chunk counts      one unsigned per kPoolListChunk pools, the non-sky pools of the chunk (the
//                     build's scratch), padded to 16 bytes
//   16 bytes          (n_nonsky, n_sky, 0, 0)
constexpr int kPoolListChunk = 4096;
constexpr size_t ao_pool_list_chunk_bytes(long long pools) {
  return (((size_t)(pools + kPoolListChunk - 1) / kPoolListChunk) * sizeof(unsigned) + 15) & ~(size_t)15;
}
constexpr size_t ao_pool_list_bytes(long long pools) { return (size_t)pools * 16 + ao_pool_list_chunk_bytes(pools) + 16; }
// blocks of a pool-list launch: one per non-sky pool, then one per 64 sky pools
constexpr long long ao_pool_list_blocks(long long n_nonsky, long long n_sky) { return n_nonsky + (n_sky + 63) / 64; }

enum KernelId { K_AOP = 1, K_POST = 2, K_AO = 3, K_PHONG = 4, K_HYBRID = 5 };

// Launch log (rt_debug_launch_log, include/rt/abi.h "Launch log"): the kernels a context launched,
// in launch order, each by its form's name: the kernel template and its arguments as the demangled
// symbol spells them, without namespaces and parameter list ("ao_batch_kernel<AoProd<16, 20, 70u>>",
// "phong_rc_kernel<true, false>", "post_kernel").  Every launcher below takes a log and appends the
// name where it picks the kernel; nullptr (the default, and every context whose log is off): one
// untaken branch per launch, no string is built.  Host code only.
struct LaunchLog {
  std::vector<std::string> names;
};

// Launch `program` (RT_PROG_* numbering) on `stream`.  Scenes with planes (p.nplanes > 0)
// take the plane-testing instantiations, scenes with rectangles in effect (p.nrects > 0, counted in
// p.nplanes too) their RC twins; every other shape is never hit (eval_ray returns -1 for it,
// p_compute.glsl:121-138) and is skipped through the NaN entries of the sphere table.  Returns hipSuccess or the launch error.
hipError_t launch_program(int program, const FrameParams& p, hipStream_t stream, LaunchLog* log = nullptr);

// Fill `table` ([ao_pool_count(p.trace_rows, p.W, p.spp)][(p.nobj + 63) / 64] u64) with the
// primary-ray cull masks an AO launch of p computes per pool: the same device functions on the same
// operands, so a launch that reads them through FrameParams::cull renders what it would have.
// They depend on p's camera, frame and strip geometry, spp, nobj and sphere rows only.
// frames: the ao_cull_frame_bytes(pools) bytes in front of `table` are written too (FrameParams::
// cull_frames): per pool the unjittered ray through its middle pixel is traced against the pool's
// own surviving spheres, and the frame is built on the hit's normal (a miss: on the reversed ray).
// Same inputs as the masks, the same values from run to run; nothing computed from a frame
// reaches a result, it only orders a pool's samples.
hipError_t launch_cull_fill(const FrameParams& p, unsigned long long* table, bool frames, hipStream_t stream,
                            LaunchLog* log = nullptr);
// Write the pool list (ao_pool_list_bytes) in front of the frames of `table`, which launch_cull_fill
// filled with frames on the same stream: two further launches of its kernel, selected by
// FrameParams::cull_frames as a mode word, one block per kPoolListChunk pools.  The first counts each
// chunk's non-sky pools; in the second every block sums the counts of the chunks before its own and
// writes its chunk's rows and sky entries in pool order, so a list is the same bytes from build to
// build.  Part of the fill: the launch log has the fill's one entry.
hipError_t launch_pool_list(const FrameParams& p, unsigned long long* table, hipStream_t stream);
// Whether an AO launch of p handed a cull table with frames may be handed the pool list as well: the
// single-frame sorted, cached forms without counters, and a pixel count a 32-bit index holds.
bool ao_takes_pool_list(const FrameParams& p);

// g-buffer layout conversion between the reference's [F][W][R] vec4 (x-major, y fastest:
// src/main.cpp:49-85 over a context's R rows) and the device slots of one array kind (0 pixels:
// [band_rows][W] float4; 1 normals: xyz plane + w plane; 2 depth: (x, y) plane + (z, w) plane),
// rows r0 .. r0 + R - 1 of the band; n = band_rows * W.  to_ref: slots -> ref, else ref -> slots.
struct GbufXfer {
  int W, R, r0, F, kind, to_ref;
  size_t n;
  float4* ref;
  float4* slot[kMaxFrames];
};
hipError_t launch_gbuf_convert(const GbufXfer& x, hipStream_t stream, LaunchLog* log = nullptr);

// The blit into an 8-bit framebuffer (rt_present): `out` = [rows][W] RGBA8 (4-byte aligned) of
// image = [rows][W] float4 by rt_quantize_rgba8's rule, output row j from image row j, or from row
// rows - 1 - j when top_down.  Four pixels per lane and 16-byte stores when W % 4 == 0 and `out` is
// 16-byte aligned, else one pixel per lane.
hipError_t launch_present(const float4* image, void* out, int W, int rows, int top_down, hipStream_t stream,
                          LaunchLog* log = nullptr);

// The blit at window size (rt_present_scaled): `out` = [out_h][out_w] RGBA8 (4-byte aligned) of
// image = [R][W] float4 sampled bilinearly with clamped edges, by rt_resample_rgba8's rule; output
// row j counts from the bottom, or from the top when top_down.  All four sizes in [1, 16384]
// (hipErrorInvalidValue otherwise).  Four pixels per lane and 16-byte stores when out_w % 4 == 0 and
// `out` is 16-byte aligned, else one pixel per lane.
hipError_t launch_present_scaled(const float4* image, int W, int R, void* out, int out_w, int out_h, int top_down,
                                 hipStream_t stream, LaunchLog* log = nullptr);

// Ray queries (include/rt/abi.h "Ray queries"): the scene and camera a query reads, as launch
// arguments.  shapes: the base of a device table copy (rt_table.h).
struct QueryScene {
  const float4* shapes;
  int S, nobj, nplanes;  // table stride, int(mode.z), planes among [0, nobj)
  float fW, fH;          // (float)W, (float)H of the whole frame
  float hx, hy, hz;      // horizontal
  float vx, vy, vz;      // vertical
  float lx, ly, lz;      // llc_minus_campos
  float cx, cy, cz;      // camera_location
  int nrects;            // rectangles in effect among the nplanes entries (in the struct's tail padding: RayQuery's
                         // members stay where they were)
};
static_assert(sizeof(QueryScene) == 80, "nrects fills QueryScene's tail padding");
// Closest hit of n rays at threshold thr (finite, >= 0), one ray per lane: the rays (origins[i],
// dirs[i]) ([n][3] each), or when xy is non-null the camera's rays through the pixels xy[i]
// ([n][2] int).  Outputs, each skipped when null: t [n], ind [n], nrm [n][3], and for pixel rays
// dir_out [n][3], the directions used.  All-sphere and with-planes instantiations, chosen from
// sc.nplanes as launch_program chooses.  n <= 2^28 (hipErrorInvalidValue otherwise); n == 0 launches nothing.
struct RayQuery {
  QueryScene sc;
  const float* origins;
  const float* dirs;
  const int* xy;
  size_t n;
  float thr;
  float* t;
  int* ind;
  float* nrm;
  float* dir_out;
};
// The query tree of the scene's spheres (include/rt/abi.h "Query tree"; rt_plan build_query_tree),
// passed beside the scene: QueryScene and RayQuery stay as they are, and so do the kernels that take
// them.  nodes: two float4 per node in preorder, the ball (centre, R) and the bits of (skip, first,
// count, 0); rows / index: the leaf table, then the n_always entries of the always list from
// always_first on.  n_nodes == 0 or a null pointer: no tree, the linear kernels.
struct QueryTree {
  const float4* nodes;
  const float4* rows;
  const int* index;
  int n_nodes, always_first, n_always;
};
// tree non-null with n_nodes > 0: ray_query_tree_kernel / occluded_tree_kernel, the same answers bit for bit
hipError_t launch_ray_query(const RayQuery& q, hipStream_t stream, const QueryTree* tree = nullptr, LaunchLog* log = nullptr);
// Occlusion of n segments from[i] -> to[i] ([n][3] each): out[i] = 1 when shadow_ray(pos = from[i],
// light = to[i]) finds an occluder (p_compute.glsl:145-166), else 0.  Same instantiations and limits.
hipError_t launch_occluded(const QueryScene& sc, const float* from, const float* to, size_t n, unsigned char* out,
                           hipStream_t stream, const QueryTree* tree = nullptr, LaunchLog* log = nullptr);

// Device math self-test (rt_selftest_math).
hipError_t launch_selftest(int fn, const float* d_in, float* d_out, size_t n, hipStream_t stream, LaunchLog* log = nullptr);

}  // namespace rt
