/*
 * rt/abi.h — C ABI of the MI355X ray-tracing hot path (librtrt.so).
 *
 * Drop-in for the GL dispatch boundary of JustinPrivitera/Real_Time_Ray_Tracer:
 *   the reference binds one std430 SSBO `shader_data` (resources/p_compute.glsl:28-63) plus
 *   an rgba32f image (src/main.cpp:389-392) and launches one of five compute programs with
 *   glDispatchCompute(WIDTH, HEIGHT, 1) from
 *     Application::compute()              src/main.cpp:553-578
 *     Application::compute_one_shader()   src/main.cpp:580-620
 *     Application::compute_two_shaders()  src/main.cpp:622-671
 *   and packs the scene / rand buffer / light with
 *     loadShapeBuffer()    src/main.cpp:395-469
 *     fill_rand_buffer()   src/main.cpp:535-539
 *     moving_light()       src/main.cpp:541-551
 *     camera basis         src/main.cpp:772-779
 *
 * Every entry point below names the reference function it replaces.  Conventions:
 *   - plain C types only; no exceptions cross the ABI;
 *   - return value 0 = RT_OK, < 0 = one of the RT_E* codes (rt_strerror() names it);
 *     functions that return a frame index return it (>= 0) on success;
 *   - one rt_ctx per (device, frame strip); a context is not thread-safe;
 *   - all GPU work is ordered on the context's HIP stream (rt_set_stream to share one).
 *
 * Host-only helpers (rt_pack_*, rt_camera_basis, rt_fill_rand_buffer, rt_moving_light,
 * rt_scenegen, rt_init_scene, rt_quantize_rgba8, rt_resample_rgba8, rt_strerror, rt_version) never
 * touch the GPU.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------------- */
enum {
  RT_OK = 0,
  RT_E_INVAL = -1,    /* bad argument (size, index, mode, program ...) */
  RT_E_NOMEM = -2,    /* host or device allocation failed */
  RT_E_HIP = -3,      /* a HIP runtime call failed; rt_last_hip_error() has the code */
  RT_E_NODEV = -4,    /* no HIP device / bad device ordinal */
  RT_E_STATE = -5     /* call order (e.g. dispatch before a header was uploaded) */
};

/* ---- compute programs (src/main.cpp:484-501, resources/<shader>.glsl) ------------------ */
enum {
  RT_PROG_AOP_COMPUTE = 1,        /* resources/aop_compute.glsl        (mode 1 pass 1) */
  RT_PROG_AOP_POSTPROCESSING = 2, /* resources/aop_postprocessing.glsl (mode 1 pass 2) */
  RT_PROG_AO_COMPUTE = 3,         /* resources/ao_compute.glsl         (mode 2)        */
  RT_PROG_P_COMPUTE = 4,          /* resources/p_compute.glsl          (mode 3)        */
  RT_PROG_H_COMPUTE = 5,          /* resources/h_compute.glsl          (mode 4)        */
  RT_PROG_COUNT = 6
};

/* ---- lighting modes (`mycam.lighting`, src/main.cpp:266-273, 553-578) -------------- */
enum { RT_MODE_AO_PP = 1, RT_MODE_AO = 2, RT_MODE_PHONG = 3, RT_MODE_PHONG_REFL = 4 };

typedef struct rt_ctx rt_ctx;

typedef struct {
  int width;      /* WIDTH  (src/main.cpp:29): full-frame width in pixels               */
  int height;     /* HEIGHT (src/main.cpp:30): full-frame height in pixels              */
  int num_shapes; /* NUM_SHAPES (src/main.cpp:34): capacity of simple_shapes[S][5]      */
  int spp;        /* AA (src/main.cpp:31): samples per pixel; rand_buffer has 2*spp vec4 */
  int num_frames; /* NUM_FRAMES (src/main.cpp:36): g-buffer ring length, normally 8     */
  int max_depth;  /* RECURSION_DEPTH (resources/ao_compute.glsl:10): path length cap, 20 (<= 65535) */
  int row_begin;  /* this context renders frame rows [row_begin, row_end);              */
  int row_end;    /*   row_begin = row_end = 0 means the whole frame                    */
} rt_config;

/* ---- context lifetime ------------------------------------------------------------- */
/* Replaces computeInitGeom()/computeInit() (src/main.cpp:471-501): allocates the device-
 * resident header, g-buffer ring (zeroed like the value-initialised ssbo_CPUMEM) and image. */
int rt_create(int device, const rt_config* cfg, rt_ctx** out);
int rt_destroy(rt_ctx* ctx);
/* Order all of the context's work on an external HIP stream (hipStream_t).  NULL is the
 * device's legacy NULL stream (e.g. torch's default stream), not "no stream". */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);
/* Go back to the context's own (non-blocking) stream. */
int rt_use_own_stream(rt_ctx* ctx);
void* rt_get_stream(rt_ctx* ctx);
/* Pipelined mode 1 (on != 0): rt_dispatch(RT_MODE_AO_PP) runs consecutive frames' aop_compute
 * passes on two alternating streams (the main stream and one of the context's own), so frame
 * k+1's pass fills the tail of frame k's, and every aop_postprocessing pass on `output_stream`
 * (NULL: a stream of the context's own).  Results are bit-identical to the sequential order:
 * normals/depth/raw pixels rotate through spare buffers and the header has two device copies,
 * so no pass sees data another in-flight pass writes.  A pipelined frame's image is complete in
 * output-stream order; rt_synchronize, rt_download and every other call (each first orders
 * all streams before the main stream) see finished frames.  Off by default. */
int rt_enable_pipelining(rt_ctx* ctx, int on, void* output_stream);
void* rt_get_output_stream(rt_ctx* ctx);
/* The stream of the last launch that wrote the context's image (the output stream for a
 * pipelined mode-1 frame, the main stream for every other program); a consumer of the image
 * (a copy, a collective) orders itself after it.  The next image writer is ordered after
 * whatever was enqueued on that stream before it. */
void* rt_image_stream(rt_ctx* ctx);
/* Number of visible HIP devices (0 when none). */
int rt_device_count(void);
/* Wait for all of the context's work (both streams). */
int rt_synchronize(rt_ctx* ctx);
int rt_last_hip_error(rt_ctx* ctx);
/* Test hook: the next query of a pinned staging buffer's "consumed" event (the uploads'
 * ring, rt_upload_header / rt_upload_rand_buffer) reports hip_error instead of asking HIP, so a
 * test can check that such a fault is returned (RT_E_HIP, rt_last_hip_error() == hip_error) and
 * the buffer is not reused.  The ring's slots are queried once they have been used (after 8
 * uploads). */
int rt_debug_fail_next_event_query(rt_ctx* ctx, int hip_error);

/* ---- device-resident path (what render() drives each frame) ------------------------ */
/* Upload the SSBO prefix: 7 header vec4 + simple_shapes[S][5] + rand_buffer[2*spp],
 * byte-identical to the reference's std430 layout (bytes == rt_header_bytes(S, spp)).
 * Replaces the memcpy-in of src/main.cpp:598-602 for everything but the g-buffer. */
int rt_upload_header(rt_ctx* ctx, const void* header, size_t bytes);
/* Replace only rand_buffer[2*spp] (fill_rand_buffer, src/main.cpp:535-539); n_vec4 == 2*spp. */
int rt_upload_rand_buffer(rt_ctx* ctx, const float* rand_vec4, size_t n_vec4);
/* Run one program on frame slot `frame` (glDispatchCompute(W,H,1), src/main.cpp:604). */
int rt_run_program(rt_ctx* ctx, int program, int frame);
/* compute() (src/main.cpp:553-578) without the host-side light/rand updates:
 * mode 1 = aop_compute + aop_postprocessing, 2 = ao_compute, 3 = p_compute, 4 = h_compute.
 * Returns the next frame slot (frame+1) % num_frames, as compute_one_shader does. */
int rt_dispatch(rt_ctx* ctx, int mode, int frame);
/* n consecutive compute() calls (src/main.cpp:553-578) as the reference's render loop makes
 * them (src/main.cpp:763-781), with the host-side updates in C++: per frame k = 0..n-1,
 * fill_rand_buffer(rand_seed + k) for the AO modes (1, 2) or moving_light(light_movement) for
 * the Phong modes (3, 4); set_mode(frame slot, int(mode.z)); upload the header; dispatch.
 * header: the caller's std430 prefix (rt_header_bytes(S, spp) bytes), updated in place as the
 * host loop leaves it.  Equal, frame for frame, to n rounds of those calls made one by one.
 * Returns the next frame slot, or < 0. */
int rt_compute_frames(rt_ctx* ctx, float* header, int mode, int frame, int n, uint64_t rand_seed,
                      int light_movement);
/* rt_compute_frames renders modes 2-4 as launches of up to `max_frames` frames (at most
 * num_frames).  1 (the default) = one launch and one image write per frame, the reference's own
 * dispatch shape (src/main.cpp:604).  > 1 = multi-frame launches (opt-in): each frame writes its
 * own ring slot, the image is written only by a launch's last frame (the one the caller sees).
 * The ring, the image the caller sees and the header are identical either way. */
int rt_set_frame_batch(rt_ctx* ctx, int max_frames);
/* Mode 4 (h_compute) tile schedule, on by default: the 16x16 tiles of a launch are dispatched
 * longest first, by the bounce rounds their waves needed in recent frames (read back every 16
 * launches on a side stream; an order is taken up once its upload has landed).  Only the order
 * of the workgroups changes, never an image.  The dispatch it replaces is the one
 * glDispatchCompute(WIDTH, HEIGHT, 1) of h_compute (src/main.cpp:604), whose workgroup order
 * the GL driver chooses.  on = 0 restores row order (and frees the schedule's buffers). */
int rt_set_tile_schedule(rt_ctx* ctx, int on);
/* 0 = off, 1 = on with row order still in use (no costs read back yet), 2 = a longest-first
 * order is in use. */
int rt_tile_schedule_state(rt_ctx* ctx);
/* how many longest-first orders have been taken up since the schedule was (re)enabled: each new
 * order replaces a table that launches still in flight may read, so tests count the swaps */
int rt_tile_schedule_orders(rt_ctx* ctx);
/* Phong g-buffer: modes 3 and 4 store normals and depth as the AO programs do.  Off by default:
 * like the reference's p_compute and h_compute, a mode-3 or mode-4 frame then writes pixels[f] and
 * the image and leaves normals_buffer[f] and depth_buffer[f] as they were (the reference's README
 * lists the stores as open work).  on != 0, per context:
 *   a mode-3 (p_compute) or mode-4 (h_compute) frame on slot f writes, for every pixel (x, y) of
 *   the rows it traces, the closest hit of the primary ray as that kernel itself found it, i.e. the
 *   surface whose colour the pixel shows (accepted for t > 0 in mode 3, p_compute.glsl:177-188, and
 *   for t > 0.001 in mode 4, h_compute.glsl:199-210):
 *     hit on shape ind at t:  normals[f][x][y] = (n, 1),  depth[f][x][y] = (t, 0, 0, 1),
 *                             n = the shading's normal of shape ind at camera + t * dir
 *                             (a sphere: normalize(p - c); a plane: its stored normal);
 *     miss:                   both are (0, 0, 0, 0).
 *   An emissive flag makes no difference (modes 3 and 4 ignore it).  These are the values
 *   ao_compute.glsl:222-229 and 249-258 write for sample 0's first segment at AA = 1.  depth.y, the
 *   AO programs' bounce count, is 0: mode 4's mirror segments are deliberately not counted there.
 *   Being g-buffer writers, the two programs then trace a strip context's band (the strip and its
 *   halo rows) for pixels, normals and depth, as the AO programs do, with the image still the
 *   strip's own rows: a strip's ring evolves like the same rows of a whole-frame ring, and a later
 *   post-process pass reads correct neighbours.  A strip's work and row counters then include the
 *   halo rows, as they do for the AO programs.  The colours do not depend on the switch.
 * A change of the switch on a strip context waits for the main stream and restarts mode 4's tile
 * schedule (a strip's tiles change with its rows); on a whole-frame context it only selects the
 * kernels of the next launch.  RT_E_INVAL for a NULL context. */
int rt_set_phong_gbuffer(rt_ctx* ctx, int on);
int rt_phong_gbuffer(rt_ctx* ctx); /* 1 = on, 0 = off */
/* Cull cache of the AO programs (modes 1 and 2), on by default.  Every pool of an AO launch starts
 * by culling the sphere table against the cone of its primary rays; that cull reads the camera,
 * the frame and strip geometry, spp, int(mode.z) and the sphere rows, none of which the render
 * loop's per-frame update changes (src/main.cpp:763-781 replaces rand_buffer and mode.y).  Once two
 * launches in a row have repeated the previous launch's values of those inputs (compared byte for
 * byte on the host), the pools' masks are written to a device table once and the launches load
 * them, until a launch's inputs differ: that launch and the next run the in-kernel cull again.  A
 * camera that moves every frame never builds a table.  Scenes with planes, and contexts whose
 * table would exceed 512 MiB or could not be allocated, always cull in the kernel.  Images, g-buffers
 * and work counters are bit-identical either way.  on = 0: every launch culls in the kernel. */
int rt_set_cull_cache(rt_ctx* ctx, int on);
/* Table fills and AO launches that loaded their masks since rt_create, and the table's bytes
 * (0 until the first fill).  Any pointer may be NULL. */
int rt_cull_cache_stats(rt_ctx* ctx, long long* fills, long long* cached_launches, size_t* table_bytes);
/* The fill also keeps, per pool, a frame on the surface normal at the hit of the pool's unjittered
 * centre ray (32 bytes per pool, allocated with the masks); the sorted AO kernels then deal the
 * pool's samples to its batches by their sector around that normal.  It changes the order of work
 * only, never a result.  When masks and frames together would exceed the cap or cannot be
 * allocated, the context keeps the masks alone.  Returns the frames' bytes (0 until the first
 * fill, and for a context that keeps masks only). */
size_t rt_cull_cache_frame_bytes(rt_ctx* ctx);
/* Test hook: this context's cap on the cull cache's bytes, in place of the build's 512 MiB
 * (0 restores it).  Before the first fill only. */
int rt_debug_cull_cache_cap(rt_ctx* ctx, size_t bytes);
/* Pool list of the cull cache, on by default.  Which pools of an AO launch are sky (no sphere in
 * their masks), and every other pool's first pixel and pixel count, depend on the cache's key alone.
 * A fill that keeps frames therefore also writes, in front of them in the same allocation (16 bytes
 * per pool, a word per 4096 pools and 16 bytes more; counted against the same cap, and left out,
 * with masks and frames kept, when the three do not fit), the non-sky pools' rows (pool, x, y,
 * pixels) and the sky pools' indices, both in ascending pool order, the same bytes for the same
 * key.  It is written by two further launches of the fill's kernel, which the launch log counts
 * with the fill's one entry.  The two counts come back to pinned host memory behind an event that
 * the launches poll and never wait for: until it has fired they run as before; from then on the
 * single-frame launches of the sorted, cached forms without counters run one workgroup per non-sky
 * pool, which reads its row in place of the pool start's divisions, and one per 64 sky pools.
 * Every other form launches as before, and so does a camera that moves every frame.  Images and
 * g-buffers are bit-identical either way.  The list follows the masks in everything else: key,
 * invalidation, streams, strips.  on = 0: no list is written or used (the key has to hold anew). */
int rt_set_pool_list(rt_ctx* ctx, int on);
/* List builds and launches over a list since rt_create, the current list's counts (-1 while there
 * is none, or its counts have not landed) and the list's bytes in the allocation (0: none).  The
 * allocation is made once, at the context's first fill, and has the list's room whenever it fits the
 * cap, also while the switch is off (the bytes are then reserved and never written), so that
 * switching the list on later needs no second allocation.  Any pointer may be NULL. */
int rt_pool_list_stats(rt_ctx* ctx, long long* builds, long long* list_launches, int* n_nonsky, int* n_sky,
                       size_t* bytes);
/* Test hook: after waiting for the device, copy to buf what the cache holds for the current key:
 * what = 0 the list's rows (16 bytes each), 1 the sky pools' indices (4 bytes each, as stored: the
 * last entry first), 2 the masks.  Returns the bytes needed (copied when they fit in cap), or a
 * negative status: RT_E_STATE without a filled table (what = 0, 1: without a list). */
long long rt_debug_pool_list_read(rt_ctx* ctx, int what, void* buf, size_t cap);
/* Launch log (test hook, off by default).  While on, the context records the form of every kernel
 * it launches, in launch order, at the point where its launcher picks the kernel: the render
 * programs, the cull cache's fill, the ray queries, the 8-bit presents, the g-buffer layout
 * conversion of rt_download / rt_upload_gbuffer and rt_selftest_math.  A form's name is the kernel
 * template and its arguments, spelled as the library's demangled symbol after one normalisation:
 * namespaces, the "void " return type and the parameter list stripped, "> >" written ">>"; for
 * instance "ao_batch_kernel<AoProd<16, 20, 70u>>", "phong_rc_kernel<true, false>", "post_kernel".
 * While off (on = 0, which also empties the log) a launch pays one untaken branch.
 * rt_debug_launch_log_read: the names so far, each followed by '\n', NUL-terminated, into buf when
 * they fit in cap bytes (then, with reset != 0, the log is emptied); returns the bytes needed, the
 * NUL included, or a negative status.  buf may be NULL with cap 0 (a size query). */
int rt_debug_launch_log(rt_ctx* ctx, int on);
long long rt_debug_launch_log_read(rt_ctx* ctx, char* buf, size_t cap, int reset);
/* Kernel forms: the AO programs' selector as the launcher calls it, for a launch of spp samples and
 * depth D over a table of ncl bounce-ray clusters, nobj objects of which nplanes are planes
 * (nrects of those rectangles in effect), with work counters, as a multi-frame launch, with a cull
 * table.  out = (sppc, dc, flags) of the form "ao_batch_kernel<AoProd<sppc, dc, flagsu>>".  Never
 * touches the GPU. */
int rt_ao_form_host(int spp, int D, int ncl, int nobj, int nplanes, int nrects, int counters, int multi_frame,
                    int cull_table, int out[3]);
/* The cull cache's key of `header` (rt_header_bytes(num_shapes, spp) bytes) for a context created
 * with `cfg`: written to `key` when it fits in key_cap bytes (key may be NULL).  Returns the key's
 * size in bytes, 0 for an invalid configuration or header.  Two launches share a table iff their
 * keys are equal.  Never touches the GPU. */
size_t rt_cull_key(const rt_config* cfg, const void* header, size_t header_bytes, void* key, size_t key_cap);
/* The bounce-ray clusters that an upload of `header` builds for a context created with `cfg` (the
 * AO kernel's later bounce rounds skip a cluster whose ball a ray provably misses).  Returns the
 * cluster count n, 0 when the cull is off for this scene, -1 for an invalid configuration or header
 * or when n > cap.  clusters[4k .. 4k+3] = cluster k's (centre, R); masks = [1 + n][4] words over the
 * sphere indices: row 0 the spheres tested in every round, row 1 + k cluster k's members.  masks
 * needs (1 + cap) * 4 words; row 0 is written when n = 0 too.  Never touches the GPU. */
int rt_cluster_table(const rt_config* cfg, const void* header, size_t header_bytes, float* clusters, uint64_t* masks,
                     int cap);
/* Copy device state to the host in the REFERENCE layout.  Any pointer may be NULL.
 * pixels/normals/depth: [F][W][R] vec4 (x-major, y fastest; R = rows of this context),
 * image: [R][W] rgba32f (row 0 = row_begin, bottom-left origin like the GL texture). */
int rt_download(rt_ctx* ctx, float* pixels, float* normals, float* depth, float* image);
/* rt_download of the window of columns [x0, x1) x frame rows [y0, y1) (inside this context's
 * rows): pixels/normals/depth as [F][x1-x0][y1-y0] vec4 (the reference's x-major, y-fastest
 * order restricted to the window), image as [y1-y0][x1-x0] rgba32f.  Any pointer may be NULL.
 * For checking regions of large frames without copying the whole ring. */
int rt_download_rect(rt_ctx* ctx, int x0, int x1, int y0, int y1, float* pixels, float* normals, float* depth,
                     float* image);
/* Upload a reference-layout g-buffer ring ([F][W][R] vec4 each; NULL = leave as is). */
int rt_upload_gbuffer(rt_ctx* ctx, const float* pixels, const float* normals, const float* depth);
/* Device pointer of the context's image ([R][W] float4), for collectives. */
void* rt_image_device_ptr(rt_ctx* ctx);
/* Render the image into a caller-owned device buffer of R*W float4 (NULL = own buffer). */
int rt_bind_image(rt_ctx* ctx, void* device_ptr);

/* ---- ray queries: closest hit, occlusion, pixel picks ----------------------------------- */
/* What does this ray hit?  The frame kernels' closest-hit scan and shadow test for the caller's own
 * rays (the reference's mouseCallback is an empty stub, src/main.cpp:286-296).
 * The scene in effect is the header last given to the context, by rt_upload_header,
 * rt_compute_frames or the host-buffer calls; nobj = int(mode.z).  Before any header: RT_E_STATE.
 * A strip context answers exactly as a whole-frame context does (scene and camera are the whole
 * frame's); no g-buffer, image or counter is touched.
 *   Closest hit of ray (o, d) at threshold thr, the reference's loop (p_compute.glsl:177-188,
 *   h_compute.glsl:199-210, ao_compute.glsl:183-194) with the threshold as a parameter:
 *     t = -1, ind = -1;  for i = 0 .. nobj-1 ascending:  res = eval_ray(o, d, i)
 *       (sphere_eval_ray for a sphere, plane_eval_ray for a plane, -1 for anything else: a
 *       rectangle is never hit unless rt_set_rectangles is on, "Rectangles" below);  if (res > thr && (res < t || t < 0)) { t = res; ind = i; }
 *   so the lowest index wins a tie.  d is used as given, NOT normalised (the sphere test assumes a
 *   unit vector, as the reference's does).  Per ray: t (float, -1 for a miss), ind (int32, -1 for a
 *   miss), normal (3 floats): zeros for a miss, the stored normal for a plane, for a sphere
 *   normalize((o + t*d) - c) with the hit point formed as one multiply and one add per component in
 *   binary32 without contraction: the value the Phong g-buffer stores for the camera's rays.  NaN
 *   and infinite operands follow the arithmetic (the sign and payload of a NaN result are not
 *   specified); a NaN res is never accepted.  thr must be finite and >= 0 (else RT_E_INVAL).
 *   Pixel rays: for integers (x, y) in frame coordinates (row 0 = the bottom row; any int32, also
 *   outside the frame) o = camera_location, d = normalize(llc_minus_campos + (x/W)*horizontal +
 *   (y/H)*vertical) (p_compute.glsl:233-235, x/W and y/H correctly rounded binary32 quotients), the
 *   ray the frame kernels trace for that pixel.  At thr = 0 the answer is what a mode-3 Phong
 *   g-buffer frame stores for the pixel, at 0.001 mode 4's, at 0.0001 the AO programs' first segment.
 *   Occlusion of the segment from a to b is shadow_ray(pos = a, light = b) (p_compute.glsl:145-166):
 *   l = normalize(b - a), len = length(b - a), o = a + 0.01f*l; occluded iff some i < nobj has
 *   t = eval_ray(o, l, i), taken as binary64, with t > 0.0001f and length(dvec3(t*l)) < len.  One
 *   byte per segment, 1 or 0.  a == b makes l NaN, and nothing occludes.
 * All float semantics as oracle/rt_oracle.h states them. */
#define RT_QUERY_MAX_RAYS ((size_t)1 << 28)
/* Host pointers; the call returns when the answers are there (it waits like rt_download).  Any
 * output pointer may be NULL; n == 0 is RT_OK.  origins / dirs / normals / from / to: [n][3] floats,
 * xy: [n][2] int32, t: [n] floats, ind: [n] int32, out: [n] bytes; rt_trace_pixels' dirs receives the
 * rays used.  RT_E_INVAL for a NULL context, a NULL input with n > 0, n > RT_QUERY_MAX_RAYS or a bad
 * thr.  The rays are staged through a device workspace of the context's own, allocated by the first
 * such call, replaced when a call needs more, freed by rt_destroy: no allocation per call. */
int rt_trace_rays(rt_ctx* ctx, const float* origins, const float* dirs, size_t n, float thr, float* t, int32_t* ind,
                  float* normals);
int rt_trace_pixels(rt_ctx* ctx, const int32_t* xy, size_t n, float thr, float* t, int32_t* ind, float* normals,
                    float* dirs);
int rt_occluded(rt_ctx* ctx, const float* from, const float* to, size_t n, uint8_t* out);
/* The same with device pointers (same layouts) on the context's device: the kernel is enqueued on
 * rt_get_stream(ctx) behind everything the context has enqueued so far (a pipelined sequence is
 * joined first), and the call returns without waiting: no allocation, no host wait, no event or
 * stream created.  A later header upload or launch is ordered after the query. */
int rt_trace_rays_device(rt_ctx* ctx, const void* d_origins, const void* d_dirs, size_t n, float thr, void* d_t,
                         void* d_ind, void* d_normals);
int rt_trace_pixels_device(rt_ctx* ctx, const void* d_xy, size_t n, float thr, void* d_t, void* d_ind,
                           void* d_normals, void* d_dirs);
int rt_occluded_device(rt_ctx* ctx, const void* d_from, const void* d_to, size_t n, void* d_out);
/* Diagnostic, like rt_cull_cache_stats: bytes of the host-pointer calls' device workspace, 0 until
 * the first of them and unchanged by a call that fits (what "no allocation per call" means; the
 * tests hold the calls to it).  Nothing else depends on it. */
size_t rt_query_workspace_bytes(rt_ctx* ctx);
/* Host only: the same rules in C on a header of rt_header_bytes(cfg->num_shapes, cfg->spp) bytes,
 * the specification of the six above; they never touch the GPU.  rt_pixel_rays_host writes the pixel
 * rays themselves (it reads cfg->width and cfg->height).  RT_E_INVAL as above, and for a header of
 * another size or an int(mode.z) outside [0, num_shapes]. */
int rt_trace_rays_host(const rt_config* cfg, const void* header, size_t header_bytes, const float* origins,
                       const float* dirs, size_t n, float thr, float* t, int32_t* ind, float* normals);
int rt_pixel_rays_host(const rt_config* cfg, const void* header, size_t header_bytes, const int32_t* xy, size_t n,
                       float* origins, float* dirs);
int rt_occluded_host(const rt_config* cfg, const void* header, size_t header_bytes, const float* from, const float* to,
                     size_t n, uint8_t* out);

/* ---- Rectangles ----------------------------------------------------------------------- */
/* The reference packs rectangles (shape id RT_SHAPE_RECTANGLE) but never intersects them: eval_ray's
 * rectangle call is commented out (resources/p_compute.glsl:132-135).  That stays the default here.
 * rt_set_rectangles(ctx, 1) makes every closest-hit loop and every shadow loop of programs 1, 3, 4
 * and 5 (modes 1-4) and of the three ray queries treat shape id 3 by the rule below; 0 restores the
 * reference's behaviour; rt_rectangles reads the switch (1 / 0).  The switch takes effect at the
 * next launch or query: the header last given to the context is packed again, and the cull cache and
 * the tile schedule start over.  A scene with no rectangle among its first int(mode.z) shapes
 * launches exactly what it launches with the switch off.
 *   The rule, for row i as loadShapeBuffer packs it (src/main.cpp:444-467): n = shapes[i][0].xyz,
 *   up = shapes[i][1].xyz, right = shapes[i][2].xyz, llc = shapes[i][3].xyz; the ray is (pos, dir),
 *   the ray's own origin and direction in every program (the AO bounces included):
 *     den = dot(n, dir);  if (den < 0.001f && den > -0.001f) return -1;    plane_eval_ray's test
 *     t   = dot(n, llc - pos) / den;                                       plane_eval_ray with p0 = llc
 *     p   = pos + t*dir;  q = p - llc;     per component one multiply, one add, one subtract, binary32,
 *                                          no contraction
 *     a   = dot(q, right);  b = dot(q, up);
 *     return (a >= 0 && a <= dot(right, right) && b >= 0 && b <= dot(up, up)) ? t : -1;
 *   dot() is the fused chain fma(z, z', fma(y, y', x*x')), `/` the IEEE division.  The edges are
 *   inclusive, both faces are hit, and a NaN anywhere fails a comparison, so the rectangle is missed.
 *   With right perpendicular to up this is the rectangle llc + u*right + v*up, u, v in [0, 1];
 *   otherwise it is the part of the plane that the two slabs 0 <= dot(q, right) <= |right|^2 and
 *   0 <= dot(q, up) <= |up|^2 enclose, a parallelogram whose sides are perpendicular to right and
 *   to up, not the one spanned by them.  The normal is the stored n, as for a plane, in shading,
 *   the g-buffers and the queries.  The tie rule (the lowest index wins) and the thresholds (0,
 *   0.001, 0.0001; shadow t > 0.0001f in binary64) are unchanged. */
#define RT_SCENE_RECTANGLES 1
int rt_set_rectangles(rt_ctx* ctx, int on);
int rt_rectangles(rt_ctx* ctx); /* 1 = on, 0 = off */
/* Host only: the rule for one packed shape row (20 floats) and one ray; the row's id is not read. */
float rt_rectangle_eval_host(const float shape[20], const float pos[3], const float dir[3]);
/* rt_trace_rays_host / rt_occluded_host with flags: RT_SCENE_RECTANGLES applies the rule to shape
 * id 3; flags = 0 is rt_trace_rays_host / rt_occluded_host.  Any other bit: RT_E_INVAL. */
int rt_trace_rays_host_ex(const rt_config* cfg, const void* header, size_t header_bytes, const float* origins,
                          const float* dirs, size_t n, float thr, int flags, float* t, int32_t* ind, float* normals);
int rt_occluded_host_ex(const rt_config* cfg, const void* header, size_t header_bytes, const float* from,
                        const float* to, size_t n, int flags, uint8_t* out);

/* ---- Query tree ----------------------------------------------------------------------- */
/* The three ray queries test every sphere for every ray.  rt_set_query_tree(ctx, 1) makes them walk
 * a tree of bounding balls over the scene's spheres instead; rt_set_query_tree(ctx, 0) restores the
 * linear scan; rt_query_tree reads the switch (1 / 0).  Off by default, and a context that never
 * switches it on allocates nothing, builds nothing and launches what it launched before.  The
 * answers are those of the linear scan, bit for bit: t, ind, normals, dirs and the occlusion bytes,
 * for every ray, NaN and infinite operands and directions of any length included.  The frame
 * programs do not use the tree.
 *   Members.  The tree is over the packed sphere rows (centre, r) of indices [0, nobj).  Rows of
 *   other shapes are left out, and so is a sphere whose radius is NaN (sphere_eval_ray gives NaN for
 *   it on every ray, so nothing ever takes it; the table packs it as such a row).  A sphere whose
 *   geometry is otherwise not finite, or whose |r| exceeds 8 times
 *   the median |r| of the finite spheres (a ground sphere), is no member: it goes to the "always"
 *   list, which every ray tests.  With fewer than 8 members (twice the leaf size, 4) no tree is
 *   built and the queries run the linear scan.
 *   Shape.  Recursive median splits of the members' centres along the widest axis, ties by index,
 *   down to leaves of 1 to 4 spheres; deterministic.  The nodes are stored in preorder, each with a
 *   ball (centre, R) and a skip link, the index of the next node that is not below it; a leaf also
 *   names a range of the leaf table (the sphere rows in leaf order, each with its index).  A
 *   traversal needs no stack: at node k it goes to k + 1 when the ray may hit the ball (after
 *   testing the members if k is a leaf), else to skip[k], and ends at the node count.
 *   Invariant.  For a leaf |c_i - centre| + |r_i| <= R for every member, for an inner node
 *   |centre_child - centre| + R_child <= R for both children (computed in binary64, rounded up), so
 *   every sphere below a node lies inside the node's ball.
 *   Node test.  The conservative ray-versus-ball test of the AO kernel's bounce clusters
 *   (RT_MATH_CULL_CLUSTER): it rejects a ball only when every sphere inside it has a negative
 *   computed discriminant or both roots negative, which no threshold >= 0 accepts and no shadow ray
 *   counts; NaN keeps the ball.  Its proof needs a unit direction, so a ray is culled only behind
 *   the unit gate: s = dot(d, d) as the fused chain fma(z, z, fma(y, y, x*x)) with
 *   |s - 1| <= 4.2e-7f.  Every normalize() result passes (pixel rays, rt_occluded's l).  A direction
 *   that fails the gate, NaN included, keeps every ball and so visits every sphere.
 *   Members, planes and rectangles are tested by the rules above ("ray queries", "Rectangles") and
 *   merged by (t, index): the candidate of least t and, among equal t, least index, which is what
 *   the ascending scan ends with.  Nothing is pruned by the closest t found so far.
 * Switching on allocates one device buffer, sized for num_shapes spheres (84 bytes per shape); no
 * later call allocates device memory for the tree (RT_E_NOMEM when it cannot be had; the switch
 * stays off).  If a header is in effect the tree is built at once.  While on, every call that gives
 * the context a header (rt_upload_header, rt_compute_frames, the host-buffer calls,
 * rt_set_rectangles) rebuilds the tree on the host and uploads it through the staging ring on
 * rt_get_stream(ctx), but only when nobj or one of the first nobj sphere rows differs, byte for
 * byte, from the last build's: a loop that moves the light or replaces rand_buffer builds once.
 * The _device queries keep their contract (no allocation, no host wait, no event or stream
 * created).  Switching off waits for the context's streams, then frees the buffer. */
int rt_set_query_tree(rt_ctx* ctx, int on);
int rt_query_tree(rt_ctx* ctx); /* 1 = on, 0 = off; RT_E_INVAL for NULL */
/* Diagnostic, like rt_cull_cache_stats: nodes, leaves and always-list entries of the tree of the
 * scene in effect (all 0 when the switch is off or the scene has no tree) and the bytes of the
 * device buffer (0 when off; unchanged by any call while on).  Any pointer may be NULL. */
int rt_query_tree_stats(rt_ctx* ctx, int* nodes, int* leaves, int* always, size_t* bytes);
/* Host only: the tree that an upload of `header` (rt_header_bytes(num_shapes, spp) bytes) builds
 * for a context created with `cfg`; never touches the GPU.  flags: 0 or RT_SCENE_RECTANGLES, as for
 * rt_trace_rays_host_ex; it does not change which rows are spheres, so the tree is the same, and any
 * other bit is refused.  Written for n nodes, e leaf entries and a always entries:
 *   balls[4k .. 4k+3] = node k's (centre, R);  links[4k .. 4k+3] = (skip, first, count, 0), count 0
 *   for an inner node, else the leaf's entries [first, first + count) of the leaf table;
 *   leaf_rows[4j .. 4j+3] = entry j's sphere row, leaf_index[j] its index;  always[0 .. a) the
 *   always list's indices, ascending.
 * Returns n, 0 when no tree is built (then e = a = 0: the linear scan tests every sphere), -1 for an
 * invalid configuration, header or flags, a NULL array, or when n > node_cap, e > leaf_cap or
 * a > always_cap.  num_shapes entries suffice for leaf_cap and always_cap, 2 * num_shapes for
 * node_cap.  n_leaf / n_always (either may be NULL) receive e and a. */
int rt_query_tree_host(const rt_config* cfg, const void* header, size_t header_bytes, int flags, float* balls,
                       int32_t* links, int node_cap, float* leaf_rows, int32_t* leaf_index, int leaf_cap,
                       int32_t* always, int always_cap, int* n_leaf, int* n_always);

/* ---- 8-bit display output (the blit, src/main.cpp:783-797) -------------------------- */
/* The reference ends a frame by drawing the rgba32f image into an 8-bit framebuffer
 * (src/main.cpp:783-797 through resources/shader_fragment.glsl:9-19: colour unchanged, alpha 1).
 * The conversion, per channel v of r, g, b in binary32 without contraction: NaN -> 0, v <= 0 -> 0,
 * v >= 1 -> 255, else (uint8)(v * 255.0f + 0.5f) truncated; the alpha byte is 255; bytes in r, g,
 * b, a order.  top_down = 0: output row j is image row j (row 0 = bottom row, like the image);
 * top_down != 0: output row j is image row R - 1 - j, the order a window or a PPM wants (for a
 * strip context R is the strip's rows and the flip is within the strip).  All opt-in: a context
 * that never calls these allocates nothing and launches nothing. */
/* Replaces the blit: enqueue the conversion of the current image (the context's own or the one
 * given to rt_bind_image) on rt_image_stream(ctx), so it reads the image after the launch that
 * wrote it and the next image writer is ordered after it.  It creates no stream and no event, and
 * returns without waiting.  The context's own 8-bit buffer is allocated (and zeroed) by the first
 * present that needs it. */
int rt_present(rt_ctx* ctx, int top_down);
/* Where the last rt_present wrote: [R][W] RGBA8 on the device; NULL before the first present. */
void* rt_present_device_ptr(rt_ctx* ctx);
/* Later presents write into a caller-owned device buffer of R*W*4 bytes, 4-byte aligned (16-byte
 * aligned for the 16-byte stores); NULL = the context's own buffer.  Does not wait for anything:
 * presents already enqueued write where they were told to. */
int rt_bind_present(rt_ctx* ctx, void* device_ptr);
/* The blit plus glReadPixels: rt_present, wait (as rt_download does), copy R*W*4 bytes to `out`. */
int rt_download_rgba8(rt_ctx* ctx, int top_down, uint8_t* out);
/* Host-only: the same conversion of image = [rows][width] rgba32f into out = [rows][width][4].  The
 * specification of rt_present in C; never touches the GPU. */
int rt_quantize_rgba8(const float* image, int width, int rows, int top_down, uint8_t* out);

/* ---- 8-bit display output at window size (the blit's scaling, src/main.cpp:381-388, 783-797) -- */
/* The reference draws the image as a textured quad into whatever framebuffer the window has
 * (glViewport every frame, src/main.cpp:783-797; the resize callback, 298-305), the texture sampled
 * with GL_LINEAR for both filters and GL_CLAMP_TO_EDGE (381-388): its screenshots are a 440x330
 * render in a 1920x1080 window.  These entry points are that blit for any output size, in either
 * direction; scaling down is plain bilinear with no mip chain, like GL_LINEAR minification.
 * The rule.  Source image = [R][W] rgba32f (row 0 = bottom row), output = [out_h][out_w] RGBA8, all
 * four sizes in [1, RT_PRESENT_SCALED_MAX].  For output column i, in 32-bit integers:
 *   n = (2*i + 1)*W - out_w, d = 2*out_w, x0 = floor(n / d), rem = n - x0*d  (0 <= rem < d),
 *   a = (float)rem / (float)d  (one correctly rounded binary32 division of two exact operands),
 *   taps = columns clamp(x0, 0, W-1) and clamp(x0 + 1, 0, W-1): clamping moves the index only, the
 *   weight stays as computed.
 * Rows likewise from R, out_h and output row j (counted from the bottom): y0, y1, b.  Per channel
 * of r, g, b in binary32 without contraction, in this order: on each of the two source rows
 *   h = (a == 0) ? t0 : ((1.0f - a)*t0 + a*t1),   then   v = (b == 0) ? h0 : ((1.0f - b)*h0 + b*h1),
 * then v is converted by rt_quantize_rgba8's rule; alpha 255; bytes r, g, b, a.  The selects on a
 * zero weight are part of the rule: at out_w == W and out_h == R every weight is 0 and the result
 * is exactly rt_present's, and a NaN or infinity under a zero weight does not reach a result.
 * top_down != 0 reverses the output rows (output row j = the bottom-up result's row out_h - 1 - j).
 * Whole-frame contexts only: the filter reads rows a strip context (rows a proper subset of the
 * frame) does not hold, so every call below returns RT_E_STATE (the pointer query NULL) for one.
 * All opt-in: a context that never calls these allocates nothing and launches nothing. */
#define RT_PRESENT_SCALED_MAX 16384
/* Enqueue the scaled blit of the current image (the context's own or rt_bind_image's) on
 * rt_image_stream(ctx), exactly where rt_present enqueues: it reads the image after the launch
 * that wrote it and the next image writer is ordered after it.  It creates no stream and no event
 * and returns without waiting.  It writes into the buffer given to rt_bind_present_scaled, else
 * into a buffer of the context's own, allocated (and zeroed) by the first scaled present that
 * needs it and kept for every size that fits.  A larger size (a window resize) replaces the own
 * buffer: before the old one is freed the call waits for all of the context's streams, as
 * rt_synchronize does; every scaled present was enqueued on one of them, so none still writes it.
 * rt_present's buffer and rt_bind_present are not touched. */
int rt_present_scaled(rt_ctx* ctx, int out_width, int out_height, int top_down);
/* Where the last rt_present_scaled wrote ([out_height][out_width] RGBA8 on the device); NULL before
 * the first. */
void* rt_present_scaled_device_ptr(rt_ctx* ctx);
/* The size of the last rt_present_scaled (RT_E_STATE before the first).  Either pointer may be NULL. */
int rt_present_scaled_size(rt_ctx* ctx, int* out_width, int* out_height);
/* Later scaled presents write into a caller-owned device buffer, 4-byte aligned (16-byte aligned for
 * the 16-byte stores), of at least out_width*out_height*4 bytes for every size the caller presents
 * at; NULL = the context's own buffer.  Does not wait for anything. */
int rt_bind_present_scaled(rt_ctx* ctx, void* device_ptr);
/* rt_present_scaled, wait (as rt_download_rgba8 does), copy out_width*out_height*4 bytes to `out`. */
int rt_download_rgba8_scaled(rt_ctx* ctx, int out_width, int out_height, int top_down, uint8_t* out);
/* Host-only: the rule above on image = [rows][width] rgba32f into out = [out_rows][out_width][4].
 * The specification of rt_present_scaled in C; never touches the GPU.  RT_E_INVAL for a NULL
 * pointer or a size outside [1, RT_PRESENT_SCALED_MAX]. */
int rt_resample_rgba8(const float* image, int width, int rows, int out_width, int out_rows, int top_down,
                      uint8_t* out);

/* ---- host-buffer parity path (mirrors the reference call shape) -------------------- */
/* compute_one_shader(frame_num, prog) (src/main.cpp:580-620): sets mode.y = frame_num in
 * `ssbo` (a whole ssbo_data-layout host buffer of rt_ssbo_bytes(S,spp,W,R,F) bytes), copies
 * it in, runs `program`, copies the g-buffer back into `ssbo`, writes the image if non-NULL,
 * and returns (frame_num + 1) % F. */
int rt_compute_one_shader(rt_ctx* ctx, void* ssbo, int frame_num, int program, float* image);
/* compute_two_shaders(frame_num, p1, p2) (src/main.cpp:622-671). */
int rt_compute_two_shaders(rt_ctx* ctx, void* ssbo, int frame_num, int program1, int program2,
                           float* image);

/* ---- multi-device row strips (one process, n strip contexts) ------------------------ */
/* The reference renders one frame with one glDispatchCompute(WIDTH, HEIGHT, 1)
 * (src/main.cpp:604, 645-653) and blits the whole image (783-797).  A group splits that frame
 * into n contiguous row strips, strip i = rows [bounds[i], bounds[i+1]) on device devices[i]
 * (devices may repeat: several strips on one GPU), each an rt_ctx with its own g-buffer ring
 * (+ 1-row halo, so strips never exchange data), and assembles the image strips into one
 * [H][W] rgba32f frame on devices[0]: root-device strips render into their frame rows, the
 * others copy their strip over xGMI (peer access) on the stream that wrote their image
 * (rt_image_stream).  One host thread per strip enqueues its work.  Results equal a
 * whole-frame rt_ctx bit for bit. */
typedef struct rt_group rt_group;
/* cfg: the whole frame (row_begin/row_end ignored); bounds: n+1 increasing rows from 0 to H,
 * or NULL for equal strips.  Fails with RT_E_NODEV for a device ordinal that does not exist and
 * when peer access from a strip's device to devices[0] cannot be enabled (the strip copies
 * would silently go through host memory). */
int rt_group_create(int n, const int* devices, const rt_config* cfg, const int* bounds, rt_group** out);
/* Strip i's copy path: 1 = its image is copied into the frame (another device, peer access
 * on, or forced below), 0 = it renders straight into its frame rows; < 0 on a bad argument. */
int rt_group_strip_copies(rt_group* g, int i);
/* Test hook: on != 0 makes every strip but the root strip (rt_group_root_strip; strip 0 unless a
 * plan moved it) render into its own image and copy it into the frame, even on the root device
 * (the copy path of distinct devices, on one GPU). */
int rt_group_force_copies(rt_group* g, int on);
int rt_group_destroy(rt_group* g);
int rt_group_size(rt_group* g);
int rt_group_bounds(rt_group* g, int* bounds);          /* n+1 entries */
/* Re-plan the strips (the contexts are re-created: fresh rings, pipelining kept). */
int rt_group_set_bounds(rt_group* g, const int* bounds);
/* Strip i's context (kernel stats, counters, downloads of its rows); owned by the group. */
rt_ctx* rt_group_strip(rt_group* g, int i);
int rt_group_last_hip_error(rt_group* g);
/* rt_enable_pipelining on every strip (each on a stream of its own). */
int rt_group_enable_pipelining(rt_group* g, int on);
/* rt_set_phong_gbuffer on every strip; kept, as pipelining is, when rt_group_set_bounds,
 * rt_group_set_plan or rt_group_balance re-create the contexts. */
int rt_group_set_phong_gbuffer(rt_group* g, int on);
/* rt_set_rectangles on every strip; kept in the same way. */
int rt_group_set_rectangles(rt_group* g, int on);
/* rt_set_query_tree on every strip; kept in the same way. */
int rt_group_set_query_tree(rt_group* g, int on);
/* rt_set_pool_list on every strip; kept in the same way. */
int rt_group_set_pool_list(rt_group* g, int on);
/* Assemble frames into a caller-owned device buffer of H*W float4 on devices[0] (NULL: the
 * group's own).  Waits for the frames in flight first. */
int rt_group_bind_frame(rt_group* g, void* device_ptr);
void* rt_group_frame_device_ptr(rt_group* g);
/* rt_upload_header for every strip (validated now, uploaded by the next dispatch). */
int rt_group_upload_header(rt_group* g, const void* header, size_t bytes);
/* compute() (src/main.cpp:553-578) on every strip + the strip copies; returns the next slot. */
int rt_group_dispatch(rt_group* g, int mode, int frame);
/* rt_compute_frames on every strip in parallel (the render loop's host updates per strip,
 * identical on all), each frame followed by the strip copies.  Returns the next slot. */
int rt_group_compute_frames(rt_group* g, float* header, int mode, int frame, int n, uint64_t rand_seed,
                            int light_movement);
int rt_group_synchronize(rt_group* g);
/* The assembled frame, [H][W] rgba32f (row 0 = bottom row, like the GL texture). */
int rt_group_download_image(rt_group* g, float* image);
/* Cost-balance the strips for `header`/`mode`: one probe frame with per-row work counters
 * gives the frame's cost profile, rt_plan_strips splits it; then `rounds` plans are timed
 * strip by strip (wall clock of 16 frames after 8, copy included) with rt_calibrate_row_cost
 * re-planning between them, and the best is kept (contexts re-created, rings fresh).
 * strip_ms (n entries, may be NULL): the kept plan's measured ms per frame per strip. */
int rt_group_balance(rt_group* g, const float* header, int mode, int rounds, double* strip_ms);
/* Host-only strip planner (no GPU): contiguous strips of nearly equal total row_cost
 * (row_cost[y] >= 0 for y < H); bounds gets n+1 entries, each strip >= 1 row. */
int rt_plan_strips(const double* row_cost, int H, int n, int* bounds);
/* Host-only gather-aware planner (no GPU).  The frame the reference blits whole
 * (src/main.cpp:783-797) is assembled on a root device that renders one strip, the root strip,
 * into its frame rows; every other strip's image (rows * width * 16 B) crosses one link into the
 * root each frame, overlapped with the next frame's render.  Minimises, over the bounds AND the
 * choice of root strip, the steady-state frame bound
 *   T = max( max_i render_i, max_{i != root} bytes_i / link_gbps, sum_{i != root} bytes_i / ingest_gbps )
 * with render_i = sum of row_ms over strip i (ms per row, e.g. rt_calibrate_row_cost's output).
 * link_gbps: GB/s one way over one link (<= 0: no link term); ingest_gbps: GB/s the root can take
 * from all links at once (<= 0: no ingest term).  Of the root positions that reach the bound, the
 * one whose strip has the most rows (fewest bytes on the links) is taken; the strips on either
 * side of it are balanced within the bound.  bounds: n+1 entries; root_strip: the strip the root
 * owns; bound_ms (NULL or 4 entries): T, render, link and ingest parts (rt_strip_gather_bound). */
int rt_plan_strips_gather(const double* row_ms, int H, int n, int width, double link_gbps, double ingest_gbps,
                          int* bounds, int* root_strip, double* bound_ms);
/* The same bound for a given plan: bound_ms[0..3] = T, max render, max link, ingest (ms). */
int rt_strip_gather_bound(const double* row_ms, int H, const int* bounds, int n, int root_strip, int width,
                          double link_gbps, double ingest_gbps, double* bound_ms);
/* Re-plan with a root strip: strip root_strip renders on devices[0] into its frame rows, strip
 * i < root_strip on devices[i + 1], strip i > root_strip on devices[i] (contexts re-created). */
int rt_group_set_plan(rt_group* g, const int* bounds, int root_strip);
int rt_group_root_strip(rt_group* g);
/* the device strip i renders on */
int rt_group_strip_device(rt_group* g, int i);
/* The link model rt_group_balance plans with when strips copy into the root (distinct devices or
 * forced copies): GB/s per link and into the root.  0 (the default) = measured by the next
 * rt_group_balance (each non-root strip's copy alone, then all at once) and kept.  The first
 * balance round plans the render only (its cost profile is not in ms yet); the gather-aware plan
 * and its root strip come from the second round on, so rounds >= 2. */
int rt_group_set_link_model(rt_group* g, double link_gbps, double ingest_gbps);
int rt_group_link_model(rt_group* g, double* link_gbps, double* ingest_gbps);
/* 8-bit output of the group (the blit of the whole frame, src/main.cpp:783-797), off by default.
 * While on, the group keeps an [H][W] RGBA8 frame on devices[0] and every strip's frame is followed
 * by rt_present on that strip: a strip that renders into the frame presents straight into its rows
 * of the 8-bit frame, every other strip copies its 8-bit strip (rows * W * 4 bytes, a quarter of
 * the float strip) on rt_image_stream in place of the float copy.  With top_down, strip i lands at
 * rows [H - bounds[i+1], H - bounds[i]).  The float frame is then no longer assembled
 * (rt_group_download_image returns RT_E_STATE), and rt_group_balance plans the copies at a quarter
 * of the bytes.  on = 0 restores the float assembly exactly.  Waits for the frames in flight. */
int rt_group_enable_rgba8(rt_group* g, int on, int top_down);
/* The assembled [H][W] RGBA8 frame (RT_E_STATE while 8-bit output is off). */
int rt_group_download_rgba8(rt_group* g, uint8_t* out);
/* The 8-bit frame on devices[0]; NULL while 8-bit output is off. */
void* rt_group_rgba8_device_ptr(rt_group* g);
/* The assembled float frame at window size, on demand (the rule of rt_present_scaled): waits for the
 * frames in flight (rt_group_synchronize), runs the scaled blit once on devices[0] over the [H][W]
 * frame and copies out_width*out_height*4 bytes to `out`.  Its device scratch is allocated by the
 * first call, regrown by a larger size and freed by rt_group_destroy.  RT_E_STATE while 8-bit
 * output is on (the float frame is not assembled then). */
int rt_group_download_rgba8_scaled(rt_group* g, int out_width, int out_height, int top_down, uint8_t* out);
/* Rescale row_cost so every strip's total equals its measured time (row shape kept). */
int rt_calibrate_row_cost(double* row_cost, int H, const int* bounds, int n, const double* strip_ms);

/* ---- instrumentation --------------------------------------------------------------- */
/* When on, every kernel launch is bracketed by HIP events on the context stream. */
int rt_enable_timing(rt_ctx* ctx, int on);
/* Sum of event-measured durations of `program`'s kernel since the last reset. */
int rt_kernel_stats(rt_ctx* ctx, int program, int* launches, double* total_ms);
int rt_reset_stats(rt_ctx* ctx);
/* Host time (ms) the context's uploads spent waiting for a free pinned staging buffer — back-
 * pressure when the host runs more than 8 uploads ahead of the GPU — and how many waits,
 * since the last rt_reset_stats.  Host time per frame minus this is the enqueue cost. */
int rt_host_stats(rt_ctx* ctx, double* wait_ms, long long* waits);
/* Work counters (a separate, un-timed instrumentation mode).  on = bit 0: totals, bit 1:
 * per-row counts.  Totals, added by every trace launch: [0] primary samples, [1] closest-hit
 * segments (one scene loop each), [2] shadow rays, [3] ray-shape tests = ([1] + [2]) *
 * int(mode.z) — the algorithmic-FLOP basis of the roofline (20 FLOP per ray-sphere test,
 * SURVEY.md §8d), [4] executed lane-tests = sum over wavefronts of 64 x the shapes their scene
 * loops tested (divergence and culling: [3]/[4] is the useful fraction; modes 3/4 count 64 x the
 * longest lane's (segments + shadow rays) x int(mode.z) per wavefront of 8 x 8 pixels; an AO pool
 * whose cull keeps no sphere runs no sphere test beyond the cull, which is then the scene loop of
 * its primary segments: 64 x the cull's rounds of the wave, ceil(int(mode.z) / 64)); post-process:
 * [5] filtered pixels (those with a primary hit, normals.w > 0.99; the others are copied),
 * [6] history slots read, [7] history slots accepted. */
int rt_enable_counters(rt_ctx* ctx, int on);
/* Read the 8 totals (synchronises); reset != 0 zeroes them afterwards. */
int rt_read_counters(rt_ctx* ctx, uint64_t out[8], int reset);
/* Per-row work of this context's rows (R = row_end - row_begin entries; a strip's halo rows are
 * traced and counted in the totals above, but not returned here), collected while row counters
 * are on.  Modes 3/4: segments + shadow rays of the row's pixels, exactly.  Modes 1/2 (the pooled
 * AO kernel): an estimate in sphere-test units, per sample of s segments
 *   kSetupCost + ncull + (s >= 2 ? b1cost + (s - 2) * nobj : 0)
 * with kSetupCost = 24 the per-sample setup, ncull <= nobj the spheres the pool's primary-ray cull
 * kept and b1cost <= nobj those the latest batched first bounce tested; a pool whose cull keeps no
 * sphere takes the empty-frustum shortcut and adds spp per pixel (1 per sample) instead.  ncull and
 * b1cost depend on the culls and on how samples are batched, not on the reference algorithm, so
 * the tests bound these rows (tests/trace_counts.py ao_row_bounds) where they check modes 3/4
 * exactly.  The cost profile used to balance row strips across GPUs. */
int rt_read_row_counters(rt_ctx* ctx, uint64_t* rows, int reset);

/* ---- device math self-test (parity of the shared float semantics) ------------------ */
enum {
  RT_MATH_SIN = 0,       /* sin used by random(): correctly rounded binary32 (in: x)  */
  RT_MATH_RANDOM = 1,    /* random(vec2) hash, p_compute.glsl:65-75 (in: x,y pairs)    */
  RT_MATH_SQRT = 2,      /* IEEE sqrt as used by the kernels (in: x)                   */
  RT_MATH_DIV = 3,       /* IEEE a/b (in: a,b pairs)                                   */
  RT_MATH_NORMALIZE = 4, /* normalize(vec3) (in: xyz triples, out: xyz triples)        */
  RT_MATH_SPHERE = 5,    /* sphere_eval_ray (in: pos3,dir3,center3,r = 10 floats)      */
  RT_MATH_SQRT_SWEEP = 6, /* out[i] = #bit patterns in [i*in[0], (i+1)*in[0]) of the
                             non-negative floats where the kernels' sqrt != sqrtf         */
  RT_MATH_RCP_SWEEP = 7,  /* out[i] = #bit patterns in [i*in[0], (i+1)*in[0]) of the non-
                             negative floats x where the kernels' 1/sqrt (normalize) differs
                             from 1.0f/sqrtf(x), plus those of the normal x in [2^-126, 2^126]
                             where their reciprocal differs from 1.0f/x                   */
  RT_MATH_SQRT_TAIL_SWEEP = 8, /* out[i] = #bit patterns in [i*in[0], (i+1)*in[0]) of the finite
                             non-negative floats where the hit-tail sqrt breaks its contract
                             (== sqrtf on [2^-96, FLT_MAX], in [0, 2^-47] below)          */
  RT_MATH_SIN_RANGE = 9,  /* out[i] = sin(x) of random() for the float whose bit pattern is
                             bits(in[0]) + i (mod 2^32): exhaustive sweeps without inputs  */
  RT_MATH_SHADOW = 10     /* shadow_ray's occluder test (p_compute.glsl:159-161) as the
                             kernels decide it: in = (light - pos).xyz, t quads; l =
                             normalize(light - pos), len = length(light - pos); out = (l.xyz,
                             len, 1 if t > 0.0001 && length(dvec3(t * l)) < len else 0)     */,
  RT_MATH_SIN_TABLE = 11, /* the sin's exception table (rt_sin_table.h) on this build's device code:
                             out[2i] = 1 if entry i's binary64 sin is flagged ambiguous (so the
                             table decides it), 0 if not, -1 past the table; out[2i+1] = its x */
  /* The kernels' conservative culls, each beside the exact test it lets them skip: the production
   * device functions themselves on the case's operands.  Decisions are 0.0 / 1.0; an accepted t is
   * that of a scan that starts at t = -1, so -1 = not accepted.  VIEW below = camera 3, llc_minus_
   * campos 3, horizontal 3, vertical 3, W, H, xmin, xmax, ymin, ymax (the pixel rectangle, inclusive),
   * hp, vp (the ray's screen position) = 20 floats. */
  RT_MATH_CULL_CAMERA = 12, /* one lane per case.  in: VIEW, sphere 4 = 24 floats.  out 7: dir 3 =
                             the primary direction at (hp, vp); miss = the rectangle's camera cone
                             excludes the sphere; t_ref = sphere_eval_ray(camera, dir); t_ao, t_p = the
                             t accepted from the sphere's camera-relative row at thresholds 0.0001, 0 */
  RT_MATH_CULL_PLANE = 13,  /* one lane per case.  in: VIEW, (n, 0), (p0, 0) = 28 floats.  out 2: miss
                             = the camera cone excludes the plane; t = plane_eval_ray(camera, dir)    */
  RT_MATH_CULL_BOUNCE = 14, /* one wavefront per case.  in: sphere 4, then per lane origin 3,
                             direction 3, live (non-zero) = 452 floats; at least one lane live.  out,
                             5 per lane = 320: miss = the live lanes' bounce cone excludes the sphere;
                             keep = its form with the pre-test row; pass = the lane's own pre-test
                             on that row (0 on lanes that are not live); t accepted at 0.0001; the t
                             that the batched first bounce's form accepts, the lanes with pass only  */
  RT_MATH_CULL_CLUSTER = 15, /* one lane per case, n a multiple of 64.  in: origin 3, direction 3,
                             cluster (centre, R) 4, member sphere 4 = 14 floats.  out 3: may = the
                             ray may hit the cluster; the lane's bit of the wave-mask form of the
                             same test; the member's t accepted at 0.0001                          */
  RT_MATH_CULL_SHADOW = 16, /* one wavefront per case.  in: light 3, sphere 4, then per lane shaded
                             point 3, need (non-zero) = 263 floats; at least one lane in need.  out,
                             2 per lane = 128: keep = the cone at the light over the needing lanes
                             does not exclude the sphere; occ = the lane's shadow ray is occluded   */
  RT_MATH_CULL_TREE = 17    /* the query tree's kernels ("Query tree").  RT_MATH_CULL_CLUSTER's cases
                             under its rule: one lane per case, n a multiple of 64, in: origin 3,
                             direction 3, ball (centre, R) 4, member sphere 4 = 14 floats.  out 3:
                             gate = the direction passes the unit gate; may = the tree kernels' node
                             decision, !gate || the cluster test; the member's t as their member test
                             accepts it from t = -1 at threshold 0 (-1: not accepted)              */
};
int rt_selftest_math(rt_ctx* ctx, int fn, const float* in, float* out, size_t n);

/* ---- host-only scene / header helpers (no GPU) ------------------------------------- */
/* loadShapeBuffer() entries (src/main.cpp:417-420, 439-442, 462-466).  `header` is the
 * SSBO prefix as float*, S its shape capacity; index i < S.  Unwritten lanes are untouched,
 * as in the reference. */
int rt_pack_sphere(float* header, int S, int i, const float center[3], float radius,
                   const float color[3], float reflectivity, int emissive);
/* plane(normal, dist, color) — p0 = dist * normal (src/geom_objs/plane.h:31-34). */
int rt_pack_plane(float* header, int S, int i, const float normal[3], float dist,
                  const float color[3], float reflectivity, int emissive);
int rt_pack_rectangle(float* header, int S, int i, const float llc[3], const float right[3],
                      const float up[3], const float color[3], float reflectivity, int emissive);
/* Camera basis of render() (src/main.cpp:772-779): w = look; u = normalize(cross(up,w));
 * v = normalize(cross(w,u)); horizontal = aspect*u; vertical = v;
 * llc_minus_campos = -0.5*(horizontal+vertical) - w; writes those + camera_location. */
int rt_camera_basis(float* header, const float location[3], const float up[3],
                    const float look_towards[3], float aspect);
/* Header fill of compute_one_shader (src/main.cpp:584-589): mode.y = frame, mode.z = n. */
int rt_set_mode(float* header, int frame, int num_objects);
/* fill_rand_buffer (src/main.cpp:535-539) with a seeded generator instead of rand():
 * splitmix64(seed), top 24 bits / 2^24 per float, 2*AA vec4. */
int rt_fill_rand_buffer(float* header, int S, int AA, uint64_t seed);
/* moving_light (src/main.cpp:541-551). */
int rt_moving_light(float* header, int light_movement);
/* Synthetic seeded scene of SURVEY §8d: ground sphere + (n_objects-1) random spheres, the
 * default camera (src/main.cpp:98-100), light (-12,8,7), SKY background, mode.z = n_objects.
 * S = capacity >= n_objects. */
int rt_scenegen(float* header, int S, int n_objects, int AA, uint64_t seed, float aspect);
/* The reference's built-in scenes 1, 5, 6 (src/scene.h:15-167) with the default camera.  7: scene
 * 5 with its light as the rectangle the reference left commented out (src/scene.h:80-86): llc
 * (4, 6, 4), right (0, 0, -8), up (-8, 0, 0), colour 1.5, emissive, in place of the emissive sphere
 * (drawn only with rt_set_rectangles on). */
int rt_init_scene(float* header, int S, int AA, int which, float aspect);

const char* rt_strerror(int status);
int rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
