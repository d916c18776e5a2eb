// rt_shim.hip — C-ABI host shim (include/rt/abi.h) over the gfx950 kernels.
//
// Replaces the GL boundary of src/main.cpp:
//   computeInitGeom / computeInit (471-501)   -> rt_create
//   compute_one_shader (580-620)              -> rt_compute_one_shader / rt_run_program
//   compute_two_shaders (622-671)             -> rt_compute_two_shaders
//   compute() (553-578)                       -> rt_dispatch
// Device layout: the g-buffer ring stays resident in HBM as per-slot row-major [rows][W]
// float4 arrays, each reached through a slot -> buffer map with spare buffers (pixels: two,
// so the post-process can write out of place and swap; normals/depth: one), instead of the
// reference's 2 x 55.76 MB host round trip per frame.  The reference [F][W][H] layout is
// produced only by rt_download / consumed by rt_upload_gbuffer.
//
// Pipelined mode 1 (rt_enable_pipelining): consecutive frames' AO passes run on two
// alternating streams (so frame k+1's AO fills the tail of frame k's), and every post-process
// runs on a third, output stream.  AO k writes its normals/depth into free buffers (a queue of
// two) and its raw pixels into one of the two spare pixel buffers, and reads its header from
// its own copy (two copies), so nothing another in-flight pass reads changes under it: the
// post-process of frame k-1 may read slot k%8's previous contents as its oldest history, and
// AO k itself reads them for the stale normal/depth of emissive first hits.  AO k waits for
// post k-2 (the last reader of the buffers it overwrites); post k waits for AO k.  The results
// are those of the sequential order, bit for bit.
//
// The subsystems are components with their own state, operations and release() (rt_stage.h,
// rt_sched.h, rt_cull.h, rt_gbuf.h, rt_timing.h, rt_query.h, rt_tree.h); the arithmetic that needs no HIP is rt_plan.cpp.
// This file keeps the context, the launches and the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/rt/abi.h"
#include "rt_cull.h"
#include "rt_gbuf.h"
#include "rt_hip_util.h"
#include "rt_kernels.h"
#include "rt_plan.h"
#include "rt_query.h"
#include "rt_sched.h"
#include "rt_stage.h"
#include "rt_timing.h"
#include "rt_tree.h"

using rt::kAoStreams;
using rt::kPipe;
static_assert(sizeof(rt::Row) == sizeof(float4) && alignof(rt::Row) == alignof(float4),
              "rt_plan packs the device table as rows of four floats");

namespace {

constexpr int kMaxShapes = 2048;
constexpr int kMaxSpp = 256;
constexpr int kMaxDepth = 65535;  // stop values are packed in 16 bits by the pooled AO kernel

}  // namespace

struct rt_ctx {
  int device = 0;
  rt_config cfg{};
  int own0 = 0, own_rows = 0;    // strip rows
  int band0 = 0, band_rows = 0;  // strip + 1-row halo (post-process neighbours)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  float4* d_shapes_buf[kAoStreams] = {};  // shape tables + rand_buffer (rt::table_vec4), one copy per AO stream
  float4* d_rb_buf[kAoStreams] = {};      // = d_shapes_buf[k] + rt::rand_table(S) (one allocation, one upload)
  float4* d_shapes = nullptr;  // the copy the next dispatch reads
  float4* d_rb = nullptr;
  // the table of the header last given to the context, which a ray query reads: d_shapes, except that
  // after a pipelined frame d_shapes moves on to the copy the next upload will fill
  const float4* d_scene = nullptr;
  // the subsystems
  rt::StageRing stage;      // pinned staging buffers of the async uploads
  rt::TileSched sched;      // mode 4's longest-first tile schedule (set up by the first hybrid launch)
  rt::CullCache cull;       // the AO pools' primary-ray cull masks while camera and scene hold
  rt::GbufRing gbuf;        // pixels / normals / depth: F slots and pipe_depth more buffers each
  rt::LaunchTiming timing;  // rt_enable_timing
  rt::QueryWork query;      // the host-pointer ray queries' device workspace (made by the first such query)
  rt::QueryTreeState tree;  // rt_set_query_tree: the queries' bounding-ball tree over the spheres (off: nothing)
  // pipelined mode 1
  bool pipelined = false;
  hipStream_t out_stream = nullptr, own_out_stream = nullptr;
  hipStream_t ao_streams[kAoStreams] = {};  // [0] unused (the main stream); [1..] the context's own
  int pipe_depth = 3, n_ao_streams = 2;
  hipEvent_t ev_ao = nullptr, ev_post[kPipe] = {}, ev_join = nullptr, ev_seq = nullptr;
  bool post_recorded[kPipe] = {};
  long long pipe_n = 0;
  bool out_pending = false;
  float4* d_image_own = nullptr;
  float4* d_image = nullptr;
  hipStream_t img_stream = nullptr;  // the stream of the last launch that wrote the image
  // rt_present: the image as [own_rows][W] RGBA8; the own buffer exists from the first present on
  unsigned char* d_present_own = nullptr;
  unsigned char* d_present_bound = nullptr;  // rt_bind_present (the caller's), else nullptr
  unsigned char* d_present = nullptr;        // where the last present wrote (nullptr before the first)
  // rt_present_scaled: the image at window size, [scaled_h][scaled_w] RGBA8; the own buffer exists
  // from the first scaled present that needs it and is replaced by one that needs more bytes
  unsigned char* d_scaled_own = nullptr;
  size_t scaled_own_bytes = 0;
  unsigned char* d_scaled_bound = nullptr;   // rt_bind_present_scaled (the caller's), else nullptr
  unsigned char* d_scaled = nullptr;         // where the last scaled present wrote
  int scaled_w = 0, scaled_h = 0;            // its size
  std::vector<float> header;   // host copy of the SSBO prefix
  std::vector<float4> table;   // host copy of the device table (rt::table_vec4 float4)
  bool have_header = false;
  int nplanes = 0;             // planes among simple_shapes[0, nobj)
  int ncl = 0;                 // AO bounce-ray clusters of the table the next dispatch reads (build_clusters)
  float4* d_xfer = nullptr;    // rt_download / rt_upload_gbuffer: one array in the reference layout [F][W][R]
  float4* d_batch = nullptr;   // rt_compute_frames: device table copies, 2 x kBatch slots (one per distinct table)
  int batch_last = -1;         // the d_batch slot d_shapes points into after rt_compute_frames (else -1)
  bool phong_gbuf = false;       // rt_set_phong_gbuffer: modes 3/4 write normals and depth, over the band
  bool rectangles = false;       // rt_set_rectangles: shape id 3 is intersected (include/rt/abi.h "Rectangles")
  int nrects = 0;                // rectangles in effect in the table the next dispatch reads (among nplanes)
  float4* d_mf_rb = nullptr;   // rt_compute_frames, mode 2: the rand_buffers of a multi-frame launch
  std::vector<float4> batch_host;
  std::vector<float> batch_hdr;  // the batch's host headers (camera, light: launch parameters)
  int nobj = 0;
  int mf_max = 1;  // rt_compute_frames: most frames per launch (rt_set_frame_batch; 1 = the reference's shape)
  unsigned long long* d_counters = nullptr;
  unsigned long long* d_row_counters = nullptr;  // [band_rows]
  bool counting = false;
  bool row_counting = false;
  int last_hip = 0;
  // rt_debug_launch_log: the forms launched while the log is on, in order; `log` is &launch_log then,
  // else nullptr (and so are cull.log and query.log): what every launcher is handed
  rt::LaunchLog launch_log;
  rt::LaunchLog* log = nullptr;
};

namespace {

using rt::hip_fail;
int hip_fail(rt_ctx* c, hipError_t e) {
  if (c) c->last_hip = (int)e;
  return RT_E_HIP;
}

size_t slot_elems(const rt_ctx* c) { return (size_t)c->band_rows * c->cfg.width; }
int table_stride(const rt_ctx* c) { return rt::table_stride(c->cfg); }
int scene_flags(const rt_ctx* c) { return c->rectangles ? RT_SCENE_RECTANGLES : 0; }
// rows of the context's table that an upload carries: the rectangle region only when some are in effect
size_t table_rows(const rt_ctx* c, int nrects) {
  return nrects > 0 ? c->table.size() : rt::table_vec4(table_stride(c), c->cfg.spp);
}
rt::Row* rows(float4* tab) { return reinterpret_cast<rt::Row*>(tab); }

int staged_copy(rt_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  return c->stage.copy(dst, src, bytes, st, c->last_hip);
}

void free_all(rt_ctx* c) {
  c->sched.release();
  c->cull.release();
  c->stage.release();
  c->timing.release();
  c->gbuf.release();
  c->query.release();
  c->tree.release();
  if (c->d_image_own) (void)hipFree(c->d_image_own);
  if (c->d_present_own) (void)hipFree(c->d_present_own);
  if (c->d_scaled_own) (void)hipFree(c->d_scaled_own);
  for (int k = 0; k < kAoStreams; ++k) {
    if (c->d_shapes_buf[k]) (void)hipFree(c->d_shapes_buf[k]);
  }
  if (c->d_counters) (void)hipFree(c->d_counters);
  if (c->d_batch) (void)hipFree(c->d_batch);
  if (c->d_xfer) (void)hipFree(c->d_xfer);
  if (c->d_mf_rb) (void)hipFree(c->d_mf_rb);
  if (c->d_row_counters) (void)hipFree(c->d_row_counters);
  for (auto e : {c->ev_ao, c->ev_join, c->ev_seq})
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->ev_post)
    if (e) (void)hipEventDestroy(e);
  if (c->own_out_stream) (void)hipStreamDestroy(c->own_out_stream);
  for (int k = 1; k < kAoStreams; ++k)
    if (c->ao_streams[k]) (void)hipStreamDestroy(c->ao_streams[k]);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
}

// the pipelined sequence is over: whatever follows is ordered after it (a join, or a drain)
void end_sequence(rt_ctx* c) {
  c->out_pending = false;
  for (auto& r : c->post_recorded) r = false;
  c->pipe_n = 0;
}

// Order everything issued so far on the output stream before later work on the main stream
// (every call except a pipelined mode-1 dispatch starts with this).
int join(rt_ctx* c) {
  if (!c->out_pending) return RT_OK;
  for (int k = 1; k < c->n_ao_streams; ++k) {
    RT_HIP(c, hipEventRecord(c->ev_join, c->ao_streams[k]));
    RT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  RT_HIP(c, hipEventRecord(c->ev_join, c->out_stream));
  RT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  end_sequence(c);  // ordered by the join from now on
  return RT_OK;
}

int sync_all(rt_ctx* c) {
  RT_HIP(c, hipStreamSynchronize(c->stream));
  for (int k = 1; k < kAoStreams; ++k)
    if (c->ao_streams[k]) RT_HIP(c, hipStreamSynchronize(c->ao_streams[k]));
  if (c->out_stream && c->out_stream != c->stream) RT_HIP(c, hipStreamSynchronize(c->out_stream));
  return RT_OK;
}

// join, then wait for all of it on the host
int drain(rt_ctx* c) {
  int rc = join(c);
  return rc == RT_OK ? sync_all(c) : rc;
}

// every stream has been drained (sync_all): forget what was in flight on them
void streams_idle(rt_ctx* c) {
  end_sequence(c);
  c->img_stream = nullptr;
  c->cull.streams_idle();
}

// Stream and header copy of the next header upload / AO pass: pipelined frames alternate
// between the main stream + copy 0 and the second stream + copy 1.
int hdr_copy(const rt_ctx* c) { return c->pipelined ? (int)(c->pipe_n % c->n_ao_streams) : 0; }
hipStream_t ao_stream(const rt_ctx* c) { return hdr_copy(c) ? c->ao_streams[hdr_copy(c)] : c->stream; }
// a new pipelined sequence: the other AO streams start after everything issued so far
int start_sequence(rt_ctx* c) {
  RT_HIP(c, hipEventRecord(c->ev_seq, c->stream));
  for (int k = 1; k < c->n_ao_streams; ++k) RT_HIP(c, hipStreamWaitEvent(c->ao_streams[k], c->ev_seq, 0));
  return RT_OK;
}

// The context has a new header (its packed table is c->table, its object count c->nobj): with the
// query tree on, rebuild and upload it if the spheres changed.  On the main stream, where the
// queries run.
int tree_update(rt_ctx* c) {
  if (!c->tree.on) return RT_OK;
  return c->tree.update(rows(c->table.data()) + rt::sphere_table(table_stride(c)), c->nobj, c->stage, c->stream,
                        c->last_hip);
}

const float* hv(const rt_ctx* c, int v) { return c->header.data() + 4 * v; }

void fill_params(const rt_ctx* c, int frame, rt::FrameParams& p) {
  std::memset(&p, 0, sizeof(p));
  p.W = c->cfg.width;
  p.H = c->cfg.height;
  p.band_row0 = c->band0;
  p.band_rows = c->band_rows;
  p.img_row0 = c->own0;
  p.img_rows = c->own_rows;
  p.nobj = c->nobj;
  p.S = table_stride(c);
  p.nplanes = c->nplanes;
  p.ncl = c->ncl;
  p.nrects = c->nrects;
  p.spp = c->cfg.spp;
  p.inv_spp = 1.0f / (float)c->cfg.spp;
  p.fW = (float)c->cfg.width;
  p.inv_W = 1.0f / p.fW;
  p.fH = (float)c->cfg.height;
  p.inv_H = 1.0f / p.fH;
  p.D = c->cfg.max_depth;
  p.F = c->cfg.num_frames;
  p.frame = frame;
  const float *h = hv(c, RT_HDR_HORIZONTAL), *v = hv(c, RT_HDR_VERTICAL),
              *l = hv(c, RT_HDR_LLC_MINUS_CAMPOS), *cam = hv(c, RT_HDR_CAMERA_LOCATION),
              *L = hv(c, RT_HDR_LIGHT_POS), *bg = hv(c, RT_HDR_BACKGROUND);
  p.hx = h[0]; p.hy = h[1]; p.hz = h[2];
  p.vx = v[0]; p.vy = v[1]; p.vz = v[2];
  p.lx = l[0]; p.ly = l[1]; p.lz = l[2];
  p.cx = cam[0]; p.cy = cam[1]; p.cz = cam[2];
  p.Lx = L[0]; p.Ly = L[1]; p.Lz = L[2];
  p.bg = make_float4(bg[0], bg[1], bg[2], bg[3]);
  p.shapes = c->d_shapes;
  p.rb = c->d_rb;
  p.image = c->d_image;
  c->gbuf.fill(p, c->cfg.num_frames, frame);
  p.counters = c->counting ? c->d_counters : nullptr;
  p.row_counters = c->row_counting ? c->d_row_counters : nullptr;
}

int launch_timed(rt_ctx* c, int program, const rt::FrameParams& p, hipStream_t st) {
  rt::LaunchTiming& t = c->timing;
  rt::LaunchTiming::Timed pair{nullptr, nullptr, p.mf_n > 0 ? p.mf_n : 1};
  if (t.on) {
    int rc = t.begin(pair, st, c->last_hip);
    if (rc != RT_OK) return rc;
  }
  RT_HIP(c, rt::launch_program(program, p, st, c->log));
  if (p.image) c->img_stream = st;  // consumers of the image order their reads after this stream
  return t.on ? t.end(program, pair, st, c->last_hip) : RT_OK;
}
// A launch of `program`; the AO passes with their cull table when the cache holds one (the fill, if
// any, goes before the timed bracket)
int launch(rt_ctx* c, int program, const rt::FrameParams& p, hipStream_t st) {
  if (program != RT_PROG_AO_COMPUTE && program != RT_PROG_AOP_COMPUTE) return launch_timed(c, program, p, st);
  rt::FrameParams q = p;
  int rc = c->cull.before(c->cfg, c->header.data(), q, st, c->last_hip);
  return rc == RT_OK ? launch_timed(c, program, q, st) : rc;
}
int launch(rt_ctx* c, int program, const rt::FrameParams& p) { return launch(c, program, p, c->stream); }

// A launch of `program` on the main stream with its tile schedule, if it has one: the hybrid
// workgroups (rt::kHyTile px square, kHyBW^2 waves) are the schedule's units.
int launch_sched(rt_ctx* c, int program, rt::FrameParams& p) {
  if (program != RT_PROG_H_COMPUTE) return launch(c, program, p);
  const int gx = (p.W + rt::kHyTile - 1) / rt::kHyTile, gy = (p.trace_rows + rt::kHyTile - 1) / rt::kHyTile;
  int rc = c->sched.before(gx, gy, rt::kHyBW * rt::kHyBW, c->stream, p, c->last_hip);
  if (rc == RT_OK) rc = launch(c, program, p);
  if (rc == RT_OK) rc = c->sched.after(c->stream, c->last_hip);
  return rc;
}

int run_program(rt_ctx* c, int program, int frame) {
  if (!c->have_header) return RT_E_STATE;
  if (frame < 0 || frame >= c->cfg.num_frames) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int jr = join(c);
  if (jr != RT_OK) return jr;
  rt::FrameParams p;
  fill_params(c, frame, p);
  switch (program) {
    case RT_PROG_P_COMPUTE:
    case RT_PROG_H_COMPUTE:
      // pixels of the strip rows only; the halo rows' pixels are never read
      p.trace_row0 = c->own0;
      p.trace_rows = c->own_rows;
      if (c->phong_gbuf) {  // a g-buffer writer like the AO programs below: the band, into the slot's buffers
        p.trace_row0 = c->band0;
        p.trace_rows = c->band_rows;
        p.phong_gbuf = 1;
      }
      p.out_pix = c->gbuf.pixels(frame);
      return launch_sched(c, program, p);
    case RT_PROG_AO_COMPUTE:
    case RT_PROG_AOP_COMPUTE:
      // g-buffer writers trace the halo rows too, so a strip's ring evolves exactly like the
      // same rows of a whole-frame ring (post-process neighbours + stale-depth reads)
      p.trace_row0 = c->band0;
      p.trace_rows = c->band_rows;
      p.out_pix = c->gbuf.pixels(frame);
      if (program == RT_PROG_AOP_COMPUTE) p.image = nullptr;  // aop_compute.glsl has no image
      return launch(c, program, p);
    case RT_PROG_AOP_POSTPROCESSING: {
      p.trace_row0 = c->own0;
      p.trace_rows = c->own_rows;
      p.raw = c->gbuf.pixels(frame);
      p.out_pix = c->gbuf.spare_pixels();
      int rc = launch(c, program, p);
      if (rc != RT_OK) return rc;
      c->gbuf.swap_spare(frame);  // filtered buffer becomes slot `frame`
      return RT_OK;
    }
    default:
      return RT_E_INVAL;
  }
}

// Frames slot0, slot0+1, ... (m <= min(kMaxBatch, F)) of one program in ONE launch: Phong /
// hybrid (gridDim.z = m, one light each) or ao_compute (gridDim.y = m, one rand_buffer each,
// from d_mf_rb).  The frames of modes 2-4 touch only their own slot (mode 2's stale-depth reads
// come from the slot's previous contents, F frames back), so they may run concurrently; the
// image, which each next frame overwrites, is written by the last frame only.
int run_program_mf(rt_ctx* c, int program, int slot0, int m, const float4* lights) {
  if (!c->have_header) return RT_E_STATE;
  if (program != RT_PROG_P_COMPUTE && program != RT_PROG_H_COMPUTE && program != RT_PROG_AO_COMPUTE) return RT_E_INVAL;
  if (m < 1 || m > rt::kMaxBatch || m > c->cfg.num_frames || slot0 < 0 || slot0 >= c->cfg.num_frames)
    return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int jr = join(c);
  if (jr != RT_OK) return jr;
  rt::FrameParams p;
  fill_params(c, slot0, p);
  const bool ao = program == RT_PROG_AO_COMPUTE;
  const bool gb = ao || c->phong_gbuf;
  p.trace_row0 = gb ? c->band0 : c->own0;  // g-buffer writers trace the halo rows too (run_program)
  p.trace_rows = gb ? c->band_rows : c->own_rows;
  p.phong_gbuf = !ao && c->phong_gbuf;  // frame j: hist_nrm / hist_dep of its slot, next to hist_pix
  p.out_pix = c->gbuf.pixels(slot0);
  p.mf_n = m;
  p.mf_slot0 = slot0;
  if (ao) p.mf_rb = c->d_mf_rb;
  else
    for (int j = 0; j < m; ++j) p.mf_light[j] = lights[j];
  return launch_sched(c, program, p);
}

// One pipelined mode-1 frame (see the header comment): AO on the frame's AO stream into free
// normals/depth buffers and a raw pixel buffer, post-process on the output stream.
int pipelined_frame(rt_ctx* c, int frame) {
  if (!c->have_header) return RT_E_STATE;
  if (frame < 0 || frame >= c->cfg.num_frames) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  const int D = c->pipe_depth;
  const int nq = (int)(c->pipe_n % D);
  hipStream_t st = ao_stream(c);
  if (c->pipe_n == 0) {  // a new sequence: the other AO streams start after everything so far
    int sr = start_sequence(c);
    if (sr != RT_OK) return sr;
  }
  if (c->post_recorded[nq]) RT_HIP(c, hipStreamWaitEvent(st, c->ev_post[nq], 0));  // post k-D
  float4* raw = c->gbuf.raw(nq);
  rt::FrameParams p;
  fill_params(c, frame, p);
  p.shapes = c->d_shapes_buf[hdr_copy(c)];
  p.rb = c->d_rb_buf[hdr_copy(c)];
  p.trace_row0 = c->band0;
  p.trace_rows = c->band_rows;
  p.out_pix = raw;
  p.image = nullptr;
  c->gbuf.fresh(p);  // (nrm_prev / dep_prev: the slot's previous contents, for the stale reads)
  int rc = launch(c, RT_PROG_AOP_COMPUTE, p, st);
  if (rc != RT_OK) return rc;
  c->gbuf.rotate(frame, D);  // the slot now maps to the fresh buffers
  RT_HIP(c, hipEventRecord(c->ev_ao, st));
  RT_HIP(c, hipStreamWaitEvent(c->out_stream, c->ev_ao, 0));
  rt::FrameParams q;
  fill_params(c, frame, q);
  q.trace_row0 = c->own0;
  q.trace_rows = c->own_rows;
  q.raw = raw;
  q.out_pix = c->gbuf.pixels(frame);  // filtered in place of slot `frame`'s oldest contents
  rc = launch(c, RT_PROG_AOP_POSTPROCESSING, q, c->out_stream);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipEventRecord(c->ev_post[nq], c->out_stream));
  c->post_recorded[nq] = true;
  c->out_pending = true;
  c->pipe_n += 1;
  c->d_shapes = c->d_shapes_buf[hdr_copy(c)];  // what a sequential dispatch would read next
  c->d_rb = c->d_rb_buf[hdr_copy(c)];
  return RT_OK;
}

int resolve_timing(rt_ctx* c) {
  if (!c->timing.any_pending()) return RT_OK;
  int rc = sync_all(c);
  return rc == RT_OK ? c->timing.resolve(c->last_hip) : rc;
}

// The g-buffer in the reference layout ([F][W][R] vec4, y fastest) goes through one device array
// of that layout: a conversion kernel (rt::launch_gbuf_convert) between it and the slot layouts,
// and one copy of exactly the caller's bytes (no host-side transposes).
// The array holds ONE frame ([W][R] vec4): frames are converted and copied one at a time (each
// frame is an independent [W][R] block of the reference layout), so a 4K context keeps 133 MB
// for it, not the ring's F frames.
int xfer_buffer(rt_ctx* c) {
  if (c->d_xfer) return RT_OK;
  return rt::alloc_or_nomem(&c->d_xfer, (size_t)c->cfg.width * c->own_rows * sizeof(float4), c->last_hip);
}
// frame f of array `kind` <-> the one-frame reference-layout array
rt::GbufXfer xfer_desc(const rt_ctx* c, int kind, int to_ref, int f) {
  rt::GbufXfer x{};
  x.W = c->cfg.width;
  x.R = c->own_rows;
  x.r0 = c->own0 - c->band0;
  x.F = 1;
  x.kind = kind;
  x.to_ref = to_ref;
  x.n = slot_elems(c);
  x.ref = c->d_xfer;
  x.slot[0] = c->gbuf.ring[kind].at(f);
  return x;
}

}  // namespace

extern "C" {

int rt_version(void) { return RT_ABI_VERSION; }

const char* rt_strerror(int s) {
  switch (s) {
    case RT_OK: return "ok";
    case RT_E_INVAL: return "invalid argument";
    case RT_E_NOMEM: return "out of memory";
    case RT_E_HIP: return "HIP runtime error";
    case RT_E_NODEV: return "no HIP device";
    case RT_E_STATE: return "bad call order";
    default: return "unknown status";
  }
}

int rt_create(int device, const rt_config* cfg, rt_ctx** out) {
  if (!cfg || !out) return RT_E_INVAL;
  *out = nullptr;
  rt_config c = *cfg;
  if (c.num_frames == 0) c.num_frames = RT_NUM_FRAMES;
  if (c.max_depth == 0) c.max_depth = RT_RECURSION_DEPTH;
  if (c.row_begin == 0 && c.row_end == 0) c.row_end = c.height;
  if (c.width <= 0 || c.height <= 0 || c.num_shapes < 0 || c.num_shapes > kMaxShapes || c.spp <= 0 ||
      c.spp > kMaxSpp || c.num_frames <= 0 || c.num_frames > rt::kMaxFrames || c.max_depth <= 0 || c.max_depth > kMaxDepth ||
      c.row_begin < 0 || c.row_end > c.height || c.row_begin >= c.row_end)
    return RT_E_INVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_E_NODEV;
  if (device < 0 || device >= ndev) return RT_E_NODEV;
  rt_ctx* x = new (std::nothrow) rt_ctx();
  if (!x) return RT_E_NOMEM;
  x->device = device;
  x->cfg = c;
  x->own0 = c.row_begin;
  x->own_rows = c.row_end - c.row_begin;
  x->band0 = std::max(0, c.row_begin - 1);
  x->band_rows = std::min(c.height, c.row_end + 1) - x->band0;
  int rc = RT_OK;
  auto fail = [&](hipError_t e) {
    x->last_hip = (int)e;
    rc = (e == hipErrorOutOfMemory) ? RT_E_NOMEM : RT_E_HIP;
  };
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&x->own_stream, hipStreamNonBlocking);
  x->stream = x->own_stream;
  const size_t slot = slot_elems(x) * sizeof(float4);
  const int F = c.num_frames;
  if (e == hipSuccess) {
    e = x->gbuf.create(F, x->pipe_depth, slot, x->stream);
    for (hipEvent_t* ev : {&x->ev_ao, &x->ev_join, &x->ev_seq})
      if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    for (auto& ev : x->ev_post)
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipMalloc(&x->d_image_own, (size_t)x->own_rows * c.width * sizeof(float4));
  if (e == hipSuccess) e = hipMemsetAsync(x->d_image_own, 0, (size_t)x->own_rows * c.width * sizeof(float4), x->stream);
  const int Sc = table_stride(x);
  for (int k = 0; k < kAoStreams; ++k) {
    if (e == hipSuccess) e = hipMalloc(&x->d_shapes_buf[k], rt::table_vec4_rect(Sc, c.spp) * sizeof(float4));
    if (e == hipSuccess) x->d_rb_buf[k] = x->d_shapes_buf[k] + rt::rand_table(Sc);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
  if (e != hipSuccess) {
    fail(e);
    free_all(x);
    delete x;
    return rc;
  }
  x->d_image = x->d_image_own;
  x->d_shapes = x->d_shapes_buf[0];
  x->d_rb = x->d_rb_buf[0];
  x->out_stream = x->own_stream;
  x->header.assign(rt_header_bytes(c.num_shapes, c.spp) / 4, 0.0f);
  x->table.assign(rt::table_vec4_rect(Sc, c.spp), make_float4(0, 0, 0, 0));  // (the rectangle rows: rt_set_rectangles)
  *out = x;
  return RT_OK;
}

int rt_destroy(rt_ctx* c) {
  if (!c) return RT_E_INVAL;
  (void)hipSetDevice(c->device);
  (void)sync_all(c);
  free_all(c);
  delete c;
  return RT_OK;
}

int rt_set_stream(rt_ctx* c, void* s) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = sync_all(c);
  if (rc != RT_OK) return rc;
  streams_idle(c);
  c->sched.forget_streams();
  c->stream = (hipStream_t)s;  // NULL = the legacy NULL stream
  if (!c->pipelined) c->out_stream = c->stream;
  // an idle own stream is released: every stream holds one of the process's few hardware
  // queues (GPU_MAX_HW_QUEUES), and busy streams that share one serialise
  if (c->own_stream && c->stream != c->own_stream && c->out_stream != c->own_stream) {
    RT_HIP(c, hipStreamDestroy(c->own_stream));
    c->own_stream = nullptr;
  }
  return RT_OK;
}

int rt_use_own_stream(rt_ctx* c) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  if (!c->own_stream) RT_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  return rt_set_stream(c, (void*)c->own_stream);
}

int rt_enable_pipelining(rt_ctx* c, int on, void* output_stream) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = sync_all(c);
  if (rc != RT_OK) return rc;
  streams_idle(c);
  c->pipelined = on != 0;
  if (!c->pipelined) {
    c->out_stream = c->stream;
    return RT_OK;
  }
  // Pipelined frames read header copy k, the first one copy 0: the table of the header last given
  // goes there when it sits elsewhere (an rt_compute_frames slot, or another copy; d_shapes itself
  // may have moved on to a copy that holds an older header, so it is not the source)
  const float4* cur = c->d_scene ? c->d_scene : c->d_shapes;
  if (cur && cur != c->d_shapes_buf[0])
    RT_HIP(c, hipMemcpyAsync(c->d_shapes_buf[0], cur, c->table.size() * sizeof(float4), hipMemcpyDeviceToDevice,
                             c->stream));
  if (cur) {
    c->d_shapes = c->d_shapes_buf[0];
    if (c->d_scene) c->d_scene = c->d_shapes;
    c->d_rb = c->d_rb_buf[0];
  }
  for (int k = 1; k < c->n_ao_streams; ++k)
    if (!c->ao_streams[k]) RT_HIP(c, hipStreamCreateWithFlags(&c->ao_streams[k], hipStreamNonBlocking));
  if (output_stream) {
    c->out_stream = (hipStream_t)output_stream;
  } else {
    if (!c->own_out_stream) RT_HIP(c, hipStreamCreateWithFlags(&c->own_out_stream, hipStreamNonBlocking));
    c->out_stream = c->own_out_stream;
  }
  if (c->out_stream == c->stream) c->pipelined = false;  // one stream: nothing to overlap
  return RT_OK;
}

void* rt_get_output_stream(rt_ctx* c) { return c ? (void*)c->out_stream : nullptr; }

void* rt_get_stream(rt_ctx* c) { return c ? (void*)c->stream : nullptr; }

void* rt_image_stream(rt_ctx* c) {
  if (!c) return nullptr;
  return (void*)(c->img_stream ? c->img_stream : c->stream);
}

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int rt_synchronize(rt_ctx* c) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  return sync_all(c);
}

int rt_last_hip_error(rt_ctx* c) { return c ? c->last_hip : 0; }

int rt_debug_fail_next_event_query(rt_ctx* c, int hip_error) {
  if (!c || hip_error == (int)hipSuccess) return RT_E_INVAL;
  c->stage.inject_query_error = hip_error;
  return RT_OK;
}

int rt_upload_header(rt_ctx* c, const void* header, size_t bytes) {
  if (!c || !header) return RT_E_INVAL;
  const int S = c->cfg.num_shapes, spp = c->cfg.spp;
  if (bytes != rt_header_bytes(S, spp)) return RT_E_INVAL;
  const float* h = (const float*)header;
  int nobj = 0, np = 0, ncl = 0, nr = 0;
  if (rt::header_nobj(h, S) < 0) return RT_E_INVAL;  // (before the context's header changes)
  if (h != c->header.data()) std::memcpy(c->header.data(), header, bytes);
  int rc = rt::pack_header(c->cfg, h, rows(c->table.data()), nobj, np, ncl, scene_flags(c), nr);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipSetDevice(c->device));
  // pipelined: into the header copy of the next frame, on its AO stream (ordered after the AO
  // pass two frames back that read that copy); sequential: in place, on the main stream
  const int hc = hdr_copy(c);
  if (c->pipelined && c->pipe_n == 0) {  // the first frame of a sequence: order after everything
    int sr = start_sequence(c);
    if (sr != RT_OK) return sr;
  }
  // table + rand_buffer in one upload (per-frame host cost matters for small strips/frames)
  // (the rectangle rows behind rand_buffer travel only when a rectangle is in effect)
  rc = staged_copy(c, c->d_shapes_buf[hc], c->table.data(), table_rows(c, nr) * sizeof(float4), ao_stream(c));
  if (rc != RT_OK) return rc;
  c->d_shapes = c->d_shapes_buf[hc];
  c->d_scene = c->d_shapes;
  c->d_rb = c->d_rb_buf[hc];
  c->nobj = nobj;
  c->nplanes = np;
  c->nrects = nr;
  c->ncl = ncl;
  c->have_header = true;
  return tree_update(c);
}

int rt_upload_rand_buffer(rt_ctx* c, const float* rb, size_t n_vec4) {
  if (!c || !rb || n_vec4 != (size_t)2 * c->cfg.spp) return RT_E_INVAL;
  std::memcpy(c->header.data() + rt_off_rand(c->cfg.num_shapes) / 4, rb, n_vec4 * 16);
  std::memcpy(c->table.data() + rt::rand_table(table_stride(c)), rb, n_vec4 * 16);
  RT_HIP(c, hipSetDevice(c->device));
  const int hc = hdr_copy(c);
  int rc = staged_copy(c, c->d_rb_buf[hc], rb, n_vec4 * 16, ao_stream(c));
  if (rc != RT_OK) return rc;
  // the other copy keeps the shape table: bring it along when switching copies
  if (c->d_shapes != c->d_shapes_buf[hc]) {
    RT_HIP(c, hipMemcpyAsync(c->d_shapes_buf[hc], c->d_shapes, rt::rand_table(table_stride(c)) * sizeof(float4),
                             hipMemcpyDeviceToDevice, ao_stream(c)));
    if (c->nrects > 0) {  // and the rectangle rows behind rand_buffer
      const size_t r0 = rt::rect_table(table_stride(c), c->cfg.spp);
      RT_HIP(c, hipMemcpyAsync(c->d_shapes_buf[hc] + r0, c->d_shapes + r0, (c->table.size() - r0) * sizeof(float4),
                               hipMemcpyDeviceToDevice, ao_stream(c)));
    }
  }
  c->d_shapes = c->d_shapes_buf[hc];
  c->d_scene = c->d_shapes;
  c->d_rb = c->d_rb_buf[hc];
  return RT_OK;
}

int rt_run_program(rt_ctx* c, int program, int frame) {
  if (!c) return RT_E_INVAL;
  return run_program(c, program, frame);
}

int rt_dispatch(rt_ctx* c, int mode, int frame) {
  if (!c) return RT_E_INVAL;
  int rc;
  switch (mode) {
    case RT_MODE_AO_PP:
      if (c->pipelined) {
        rc = pipelined_frame(c, frame);
        break;
      }
      rc = run_program(c, RT_PROG_AOP_COMPUTE, frame);
      if (rc == RT_OK) rc = run_program(c, RT_PROG_AOP_POSTPROCESSING, frame);
      break;
    case RT_MODE_AO: rc = run_program(c, RT_PROG_AO_COMPUTE, frame); break;
    case RT_MODE_PHONG: rc = run_program(c, RT_PROG_P_COMPUTE, frame); break;
    case RT_MODE_PHONG_REFL: rc = run_program(c, RT_PROG_H_COMPUTE, frame); break;
    default: return RT_E_INVAL;
  }
  if (rc != RT_OK) return rc;
  return (frame + 1) % c->cfg.num_frames;
}

int rt_compute_frames(rt_ctx* c, float* header, int mode, int frame, int n, uint64_t rand_seed, int light_movement) {
  if (!c || !header || n < 0 || mode < RT_MODE_AO_PP || mode > RT_MODE_PHONG_REFL) return RT_E_INVAL;
  if (frame < 0 || frame >= c->cfg.num_frames) return RT_E_INVAL;
  const int S = c->cfg.num_shapes, spp = c->cfg.spp;
  const size_t bytes = rt_header_bytes(S, spp);
  // the render loop's host update of frame k (src/main.cpp:553-578), then set_mode
  auto update = [&](int k, int slot) -> int {
    int rc = (mode == RT_MODE_AO_PP || mode == RT_MODE_AO) ? rt_fill_rand_buffer(header, S, spp, rand_seed + (uint64_t)k)
                                                           : rt_moving_light(header, light_movement);
    if (rc != RT_OK) return rc;
    const int nobj = rt::header_nobj(header, S);
    return nobj < 0 ? RT_E_INVAL : rt_set_mode(header, slot, nobj);
  };
  // Multi-frame launches (run_program_mf): the shape table is uploaded once and up to kMaxBatch
  // frames go in one launch.
  // Modes 3/4: the per-frame host update moves only the light (and mode.y), so the frames go with
  // their lights.  Every frame writes its own colour slot, as frame-by-frame calls do; the image is
  // written once per launch, by its last frame (the one the caller sees).
  // Mode 2: the per-frame host update replaces only rand_buffer (fill_rand_buffer,
  // src/main.cpp:535-539) and mode.y, so each frame goes with its own rand_buffer.
  const bool mf_light = (mode == RT_MODE_PHONG || mode == RT_MODE_PHONG_REFL) && n >= 2 && c->mf_max > 1;
  const bool mf_rand = mode == RT_MODE_AO && n >= 2 && !c->counting && !c->row_counting && c->mf_max > 1;
  if (mf_light || mf_rand) {
    const size_t per = mf_rand ? (size_t)2 * spp : 1;  // float4 per frame: its rand_buffer, or its light
    const float* src = header + (mf_rand ? rt_off_rand(S) / 4 : 4 * RT_HDR_LIGHT_POS);
    std::vector<float4> vals((size_t)n * per);
    std::vector<int> slots(n);
    int f = frame;
    for (int k = 0; k < n; ++k) {
      int rc = update(k, f);
      if (rc == RT_OK && k == 0) rc = rt_upload_header(c, header, bytes);
      if (rc != RT_OK) return rc;
      std::memcpy(&vals[(size_t)k * per], src, per * sizeof(float4));
      slots[k] = f;
      f = (f + 1) % c->cfg.num_frames;
    }
    if (mf_rand) {
      RT_HIP(c, hipSetDevice(c->device));
      if (!c->d_mf_rb) RT_HIP(c, hipMalloc(&c->d_mf_rb, (size_t)rt::kMaxBatch * per * sizeof(float4)));
    } else {
      std::memcpy(c->header.data(), header, bytes);  // as the per-frame calls leave it
    }
    const int prog = mode == RT_MODE_AO ? RT_PROG_AO_COMPUTE : mode == RT_MODE_PHONG ? RT_PROG_P_COMPUTE : RT_PROG_H_COMPUTE;
    // at most F frames per launch: each colour slot is written by one frame of a launch (frames
    // k and k + F of one launch would race for slot k % F)
    const int mb = std::min(std::min(rt::kMaxBatch, c->mf_max), c->cfg.num_frames);
    for (int k0 = 0; k0 < n; k0 += mb) {
      const int m = std::min(mb, n - k0);
      const float4* v = &vals[(size_t)k0 * per];
      int rc = mf_rand ? staged_copy(c, c->d_mf_rb, v, (size_t)m * per * sizeof(float4), c->stream) : RT_OK;
      if (rc == RT_OK) rc = run_program_mf(c, prog, slots[k0], m, mf_rand ? nullptr : v);
      if (rc != RT_OK) return rc;
    }
    // mode 2 leaves the context as the per-frame calls would: the last header uploaded
    int rc = mf_rand ? rt_upload_header(c, header, bytes) : RT_OK;
    return rc == RT_OK ? f : rc;
  }
  if (c->pipelined || n < 2) {  // pipelined mode 1 rotates its own header copies per frame
    for (int k = 0; k < n; ++k) {
      int rc = update(k, frame);
      if (rc == RT_OK) rc = rt_upload_header(c, header, bytes);
      if (rc != RT_OK) return rc;
      frame = rt_dispatch(c, mode, frame);
      if (frame < 0) return frame;
    }
    return frame;
  }
  // Sequential frames in batches: the host updates of up to kBatch frames are packed into
  // device table copies with ONE upload, then the frames' programs are launched back to back,
  // each reading its own copy.  Per frame the host then only enqueues kernels, which keeps small
  // frames (config (a): a ~9 us kernel) GPU-bound.  Only DISTINCT tables are uploaded: modes 3/4
  // move the light, which travels in the kernel arguments, so their packed table never changes
  // and, after the first call, nothing is copied at all (an in-stream host-to-device copy
  // between two kernels stalls the queue for the copy's round trip: ~40 us every 8 frames of
  // config (b), 5 us per frame).  The last table stays where it is (d_batch slot batch_last)
  // as the context's current table.
  constexpr int kBatch = 32;
  const size_t tv = c->table.size();
  RT_HIP(c, hipSetDevice(c->device));
  int jr = join(c);
  if (jr != RT_OK) return jr;
  if (!c->d_batch) RT_HIP(c, hipMalloc(&c->d_batch, (size_t)2 * kBatch * tv * sizeof(float4)));
  c->batch_host.resize((size_t)kBatch * tv);
  c->batch_hdr.resize((size_t)kBatch * (bytes / sizeof(float)));
  const int Sc = table_stride(c);
  const size_t hf = bytes / sizeof(float);
  const size_t tb = tv * sizeof(float4);
  for (int k0 = 0; k0 < n; k0 += kBatch) {
    const int m = std::min(kBatch, n - k0);
    std::vector<int> nobj(m), npl(m), ncl(m), nrc(m), slot(m), dslot(m);
    std::vector<unsigned char> same(m);  // frame j's table equals the previous frame's
    // the context's current table, if it already sits in a d_batch slot (host copy: c->table)
    const int prev = (c->batch_last >= 0 && c->d_shapes == c->d_batch + (size_t)c->batch_last * tv) ? c->batch_last : -1;
    int nd = 0;                  // distinct new tables, packed into batch_host[0 .. nd)
    const float4* last = prev >= 0 ? c->table.data() : nullptr;  // the previous frame's table
    int f = frame;
    for (int j = 0; j < m; ++j) {
      float4* tab = c->batch_host.data() + (size_t)nd * tv;
      int rc = update(k0 + j, f);
      if (rc == RT_OK) rc = rt::pack_header(c->cfg, header, rows(tab), nobj[j], npl[j], ncl[j], scene_flags(c), nrc[j]);
      if (rc != RT_OK) return rc;
      std::memcpy(c->batch_hdr.data() + (size_t)j * hf, header, bytes);  // camera / light of frame j
      slot[j] = f;
      f = (f + 1) % c->cfg.num_frames;
      same[j] = last && std::memcmp(tab, last, tb) == 0;
      if (!same[j]) {
        last = tab;
        ++nd;
      }
    }
    const int base = rt::batch_slots(same.data(), m, prev, 2 * kBatch, dslot.data());
    if (nd > 0) {
      int rc = staged_copy(c, c->d_batch + (size_t)base * tv, c->batch_host.data(), (size_t)nd * tb, c->stream);
      if (rc != RT_OK) return rc;
    }
    // the context's table from here on: the last frame's (host copy first: `last` may point
    // into batch_host, which the next batch reuses)
    if (last != c->table.data()) std::memcpy(c->table.data(), last, tb);
    for (int j = 0; j < m; ++j) {
      c->d_shapes = c->d_batch + (size_t)dslot[j] * tv;
      c->d_scene = c->d_shapes;
      c->d_rb = c->d_shapes + rt::rand_table(Sc);
      c->nobj = nobj[j];
      c->nplanes = npl[j];
      c->nrects = nrc[j];
      c->ncl = ncl[j];
      c->have_header = true;
      std::memcpy(c->header.data(), c->batch_hdr.data() + (size_t)j * hf, bytes);  // launch parameters
      frame = rt_dispatch(c, mode, slot[j]);
      if (frame < 0) return frame;
    }
    c->batch_last = dslot[m - 1];
  }
  // the context is left as the per-frame calls would leave it: the last header, its table current
  std::memcpy(c->header.data(), header, bytes);
  int tr = tree_update(c);  // (the frames' tables never went through rt_upload_header)
  if (tr != RT_OK) return tr;
  return frame;
}

int rt_set_tile_schedule(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the tables freed here
  c->sched.release();
  c->sched.on = on != 0;
  return RT_OK;
}

int rt_set_phong_gbuffer(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  if (c->phong_gbuf == (on != 0)) return RT_OK;
  if (c->band0 != c->own0 || c->band_rows != c->own_rows) {
    // a strip's mode-4 launches change their rows, so their tiles: the schedule's costs and order
    // restart, as on rt_set_tile_schedule (no launch in flight reads the tables freed here)
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->sched.release();
  }
  c->phong_gbuf = on != 0;
  return RT_OK;
}

int rt_phong_gbuffer(rt_ctx* c) { return c ? (c->phong_gbuf ? 1 : 0) : RT_E_INVAL; }

int rt_set_rectangles(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  if (c->rectangles == (on != 0)) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = drain(c);  // no launch in flight reads the tables replaced or freed here
  if (rc != RT_OK) return rc;
  streams_idle(c);
  c->rectangles = on != 0;
  // what depended on the old table starts over: the cull cache's key and masks, the tile schedule's
  // costs and order, and the packed table itself (the header last given, packed and uploaded again)
  c->sched.release();
  c->cull.have_key = false;
  rc = c->cull.invalidate(c->last_hip);
  if (rc != RT_OK) return rc;
  c->batch_last = -1;
  if (c->have_header) rc = rt_upload_header(c, c->header.data(), c->header.size() * sizeof(float));
  return rc;
}

int rt_rectangles(rt_ctx* c) { return c ? (c->rectangles ? 1 : 0) : RT_E_INVAL; }

int rt_set_query_tree(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  if (c->tree.on == (on != 0)) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  if (!on) {
    int rc = drain(c);  // no query in flight reads the buffer freed here
    if (rc != RT_OK) return rc;
    streams_idle(c);
    c->tree.release();
    return RT_OK;
  }
  int rc = c->tree.enable(c->cfg.num_shapes, c->last_hip);
  if (rc != RT_OK) return rc;
  return c->have_header ? tree_update(c) : RT_OK;
}

int rt_query_tree(rt_ctx* c) { return c ? (c->tree.on ? 1 : 0) : RT_E_INVAL; }

int rt_query_tree_stats(rt_ctx* c, int* nodes, int* leaves, int* always, size_t* bytes) {
  if (!c) return RT_E_INVAL;
  const bool built = c->tree.on && c->tree.n_nodes > 0;
  if (nodes) *nodes = built ? c->tree.n_nodes : 0;
  if (leaves) *leaves = built ? c->tree.host.n_leaves : 0;
  if (always) *always = built ? c->tree.host.n_always : 0;
  if (bytes) *bytes = c->tree.bytes;
  return RT_OK;
}

int rt_tile_schedule_state(rt_ctx* c) {
  if (!c) return RT_E_INVAL;
  if (!c->sched.on) return 0;
  return c->sched.active >= 0 ? 2 : 1;
}

int rt_tile_schedule_orders(rt_ctx* c) { return c ? c->sched.orders_taken : RT_E_INVAL; }

int rt_set_cull_cache(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  c->cull.on = on != 0;
  c->cull.have_key = false;  // on again: the key has to hold anew
  return c->cull.invalidate(c->last_hip);
}

int rt_debug_cull_cache_cap(rt_ctx* c, size_t bytes) {
  if (!c) return RT_E_INVAL;
  if (c->cull.d_alloc) return RT_E_INVAL;  // before the first fill
  c->cull.cap = bytes && bytes < rt::kCullCacheMaxBytes ? bytes : rt::kCullCacheMaxBytes;
  return RT_OK;
}

size_t rt_cull_cache_frame_bytes(rt_ctx* c) { return c ? c->cull.frame_bytes : 0; }

int rt_set_pool_list(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  if (c->cull.list_on == (on != 0)) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  c->cull.list_on = on != 0;
  c->cull.have_key = false;  // the next fill writes the list (or none): the key has to hold anew
  return c->cull.invalidate(c->last_hip);
}

int rt_pool_list_stats(rt_ctx* c, long long* builds, long long* list_launches, int* n_nonsky, int* n_sky, size_t* bytes) {
  if (!c) return RT_E_INVAL;
  const rt::CullCache& k = c->cull;
  if (builds) *builds = k.list_builds;
  if (list_launches) *list_launches = k.list_launches;
  if (n_nonsky) *n_nonsky = k.list_ready ? k.h_counts[0] : -1;
  if (n_sky) *n_sky = k.list_ready ? k.h_counts[1] : -1;
  if (bytes) *bytes = k.list_bytes;
  return RT_OK;
}

long long rt_debug_pool_list_read(rt_ctx* c, int what, void* buf, size_t cap) {
  if (!c || what < 0 || what > 2 || (!buf && cap)) return RT_E_INVAL;
  const rt::CullCache& k = c->cull;
  if (!k.valid || (what != 2 && (k.list_bytes == 0 || !(k.list_pending || k.list_ready)))) return RT_E_STATE;
  RT_HIP(c, hipSetDevice(c->device));
  RT_HIP(c, hipDeviceSynchronize());  // the fill and the list's build have run
  const char* const list = (const char*)k.d_alloc;
  const size_t rows_cap = (size_t)k.list_pools * 16;  // the sky list ends where the rows' bytes end
  const char* src = (const char*)k.d_table;
  size_t need = k.bytes;
  if (what != 2) {
    int counts[4];
    RT_HIP(c, hipMemcpy(counts, (const char*)k.d_table - k.frame_bytes - 16, sizeof counts, hipMemcpyDeviceToHost));
    need = what == 0 ? (size_t)counts[0] * 16 : (size_t)counts[1] * 4;
    src = what == 0 ? list : list + rows_cap - need;
  }
  if (need <= cap && need) RT_HIP(c, hipMemcpy(buf, src, need, hipMemcpyDeviceToHost));
  return (long long)need;
}

int rt_debug_launch_log(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  c->log = on ? &c->launch_log : nullptr;
  c->cull.log = c->log;
  c->query.log = c->log;
  if (!on) c->launch_log.names.clear();
  return RT_OK;
}

long long rt_debug_launch_log_read(rt_ctx* c, char* buf, size_t cap, int reset) {
  if (!c || (!buf && cap)) return RT_E_INVAL;
  size_t need = 1;  // the terminating NUL
  for (const auto& s : c->launch_log.names) need += s.size() + 1;
  if (need <= cap) {
    char* p = buf;
    for (const auto& s : c->launch_log.names) {
      std::memcpy(p, s.data(), s.size());
      p += s.size();
      *p++ = '\n';
    }
    *p = 0;
    if (reset) c->launch_log.names.clear();
  }
  return (long long)need;
}

int rt_cull_cache_stats(rt_ctx* c, long long* fills, long long* cached_launches, size_t* table_bytes) {
  if (!c) return RT_E_INVAL;
  if (fills) *fills = c->cull.fills;
  if (cached_launches) *cached_launches = c->cull.cached;
  if (table_bytes) *table_bytes = c->cull.bytes;
  return RT_OK;
}

size_t rt_cull_key(const rt_config* cfg, const void* header, size_t header_bytes, void* key, size_t key_cap) {
  if (!cfg || !header || cfg->width <= 0 || cfg->height <= 0 || cfg->spp <= 0 || cfg->num_shapes < 0 ||
      header_bytes != rt_header_bytes(cfg->num_shapes, cfg->spp))
    return 0;
  rt_config x = *cfg;
  if (x.row_begin == 0 && x.row_end == 0) x.row_end = x.height;  // as rt_create
  if (x.row_begin < 0 || x.row_end > x.height || x.row_begin >= x.row_end) return 0;
  return rt::cull_key(x, (const float*)header, (unsigned char*)key, key_cap);
}

int rt_cluster_table(const rt_config* cfg, const void* header, size_t header_bytes, float* clusters, uint64_t* masks,
                     int cap) {
  if (!cfg || !header || !clusters || !masks || cap < 0 || cfg->spp <= 0 || cfg->num_shapes < 0 ||
      header_bytes != rt_header_bytes(cfg->num_shapes, cfg->spp))
    return -1;
  // the table an upload packs (pack_header: the sphere table, then build_clusters over it)
  const int Sc = rt::table_stride(*cfg);
  std::vector<float4> tab(rt::table_vec4(Sc, cfg->spp));
  int nobj = 0, np = 0, ncl = 0;
  if (rt::pack_header(*cfg, (const float*)header, rows(tab.data()), nobj, np, ncl) != RT_OK || ncl > cap) return -1;
  std::memcpy(clusters, tab.data() + rt::cluster_table(Sc), (size_t)ncl * sizeof(float4));
  std::memcpy(masks, tab.data() + rt::cluster_mask_table(Sc), (size_t)(1 + ncl) * rt::kClusterWords * sizeof(uint64_t));
  return ncl;
}

int rt_set_frame_batch(rt_ctx* c, int max_frames) {
  if (!c || max_frames < 1) return RT_E_INVAL;
  c->mf_max = std::min(max_frames, rt::kMaxBatch);
  return RT_OK;
}

int rt_download(rt_ctx* c, float* pixels, float* normals, float* depth, float* image) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = drain(c);
  if (rc == RT_OK && (pixels || normals || depth)) rc = xfer_buffer(c);
  if (rc != RT_OK) return rc;
  const size_t fbytes = (size_t)c->cfg.width * c->own_rows * sizeof(float4);  // one frame
  float* dst[3] = {pixels, normals, depth};
  for (int k = 0; k < 3; ++k) {
    if (!dst[k]) continue;
    for (int f = 0; f < c->cfg.num_frames; ++f) {  // stream order: frame f's copy precedes f+1's convert
      RT_HIP(c, rt::launch_gbuf_convert(xfer_desc(c, k, 1, f), c->stream, c->log));
      RT_HIP(c, hipMemcpyAsync((char*)dst[k] + (size_t)f * fbytes, c->d_xfer, fbytes, hipMemcpyDeviceToHost,
                               c->stream));
    }
  }
  if (image)
    RT_HIP(c, hipMemcpyAsync(image, c->d_image, (size_t)c->own_rows * c->cfg.width * 16, hipMemcpyDeviceToHost,
                             c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_download_rect(rt_ctx* c, int x0, int x1, int y0, int y1, float* pixels, float* normals, float* depth,
                     float* image) {
  if (!c) return RT_E_INVAL;
  const int W = c->cfg.width;
  if (x0 < 0 || x1 > W || x0 >= x1 || y0 < c->own0 || y1 > c->own0 + c->own_rows || y0 >= y1) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = drain(c);
  if (rc != RT_OK) return rc;
  const int w = x1 - x0, h = y1 - y0, F = c->cfg.num_frames;
  const size_t pitch = (size_t)W * sizeof(float4), row = (size_t)w * sizeof(float4);
  std::vector<float4> tmp((size_t)w * h);
  auto rect = [&](const float4* base, int r0) {  // rows [r0, r0 + h) of a [rows][W] device array
    return hipMemcpy2D(tmp.data(), row, base + (size_t)r0 * W + x0, pitch, row, h, hipMemcpyDeviceToHost);
  };
  // a plane-split slot's rect: plane a (ea floats per pixel) then plane b (4 - ea floats per
  // pixel, starting ea * n floats into the slot), interleaved into tmp
  const size_t n = slot_elems(c);
  std::vector<float> ta((size_t)w * h * 3), tb((size_t)w * h * 3);
  auto split_rect = [&](const float4* base, int r0, int ea) -> hipError_t {
    const int eb = 4 - ea;
    const float* pa = (const float*)base + ((size_t)r0 * W + x0) * ea;
    const float* pb = (const float*)base + ea * n + ((size_t)r0 * W + x0) * eb;
    hipError_t e = hipMemcpy2D(ta.data(), (size_t)w * ea * 4, pa, (size_t)W * ea * 4, (size_t)w * ea * 4, h,
                               hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy2D(tb.data(), (size_t)w * eb * 4, pb, (size_t)W * eb * 4, (size_t)w * eb * 4, h,
                      hipMemcpyDeviceToHost);
    for (size_t i = 0; i < (size_t)w * h; ++i) {
      float* o = (float*)&tmp[i];
      for (int q = 0; q < ea; ++q) o[q] = ta[i * ea + q];
      for (int q = 0; q < eb; ++q) o[ea + q] = tb[i * eb + q];
    }
    return e;
  };
  for (int f = 0; f < F; ++f) {
    float* const dst[rt::kSlotKinds] = {pixels, normals, depth};
    for (int k = 0; k < rt::kSlotKinds; ++k) {
      if (!dst[k]) continue;
      const float4* src = c->gbuf.ring[k].at(f);
      RT_HIP(c, (k == rt::kPixels || (k == rt::kNormals && !RT_NRM_PLANES)) ? rect(src, y0 - c->band0)
                                                                           : split_rect(src, y0 - c->band0, k == rt::kNormals ? 3 : 2));
      float* out = dst[k] + (size_t)f * w * h * 4;  // [w][h] vec4, y fastest (reference layout)
      for (int x = 0; x < w; ++x)
        for (int r = 0; r < h; ++r) std::memcpy(out + ((size_t)x * h + r) * 4, &tmp[(size_t)r * w + x], 16);
    }
  }
  if (image) {
    RT_HIP(c, rect(c->d_image, y0 - c->own0));
    std::memcpy(image, tmp.data(), tmp.size() * sizeof(float4));
  }
  return RT_OK;
}

int rt_upload_gbuffer(rt_ctx* c, const float* pixels, const float* normals, const float* depth) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = drain(c);
  if (rc == RT_OK && (pixels || normals || depth)) rc = xfer_buffer(c);
  if (rc != RT_OK) return rc;
  const size_t fbytes = (size_t)c->cfg.width * c->own_rows * sizeof(float4);  // one frame
  const float* src[3] = {pixels, normals, depth};
  for (int k = 0; k < 3; ++k) {  // (the halo rows of a strip keep their contents)
    if (!src[k]) continue;
    for (int f = 0; f < c->cfg.num_frames; ++f) {
      RT_HIP(c, hipMemcpyAsync(c->d_xfer, (const char*)src[k] + (size_t)f * fbytes, fbytes, hipMemcpyHostToDevice,
                               c->stream));
      RT_HIP(c, rt::launch_gbuf_convert(xfer_desc(c, k, 0, f), c->stream, c->log));
    }
  }
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

void* rt_image_device_ptr(rt_ctx* c) { return c ? (void*)c->d_image : nullptr; }

int rt_bind_image(rt_ctx* c, void* p) {
  if (!c) return RT_E_INVAL;
  c->d_image = p ? (float4*)p : c->d_image_own;
  return RT_OK;
}

// ---- the blit (src/main.cpp:783-797) ----------------------------------------------------
int rt_present(rt_ctx* c, int top_down) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  // on the stream of the last launch that wrote the image: the conversion reads the image after
  // that launch, and the next image writer is ordered after this stream's work (rt_image_stream)
  hipStream_t st = (hipStream_t)rt_image_stream(c);
  const size_t bytes = (size_t)c->own_rows * c->cfg.width * 4;
  unsigned char* dst = c->d_present_bound;
  if (!dst) {
    if (!c->d_present_own) {
      int rc = rt::alloc_or_nomem(&c->d_present_own, bytes, c->last_hip);
      if (rc != RT_OK) return rc;
      RT_HIP(c, hipMemsetAsync(c->d_present_own, 0, bytes, st));
    }
    dst = c->d_present_own;
  }
  RT_HIP(c, rt::launch_present(c->d_image, dst, c->cfg.width, c->own_rows, top_down != 0, st, c->log));
  c->d_present = dst;
  return RT_OK;
}

void* rt_present_device_ptr(rt_ctx* c) { return c ? (void*)c->d_present : nullptr; }

int rt_bind_present(rt_ctx* c, void* p) {
  if (!c || ((uintptr_t)p & 3)) return RT_E_INVAL;  // the kernel stores whole pixels
  c->d_present_bound = (unsigned char*)p;
  return RT_OK;
}

int rt_download_rgba8(rt_ctx* c, int top_down, uint8_t* out) {
  if (!c || !out) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = rt_present(c, top_down);
  if (rc == RT_OK) rc = drain(c);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipMemcpyAsync(out, c->d_present, (size_t)c->own_rows * c->cfg.width * 4, hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---- the blit at window size (src/main.cpp:381-388, 783-797) --------------------------------
// the filter reads rows above and below an output row's: whole-frame contexts only
static bool whole_frame(const rt_ctx* c) { return c->own0 == 0 && c->own_rows == c->cfg.height; }
static bool scaled_size_ok(int w, int h) {
  return w >= 1 && h >= 1 && w <= RT_PRESENT_SCALED_MAX && h <= RT_PRESENT_SCALED_MAX;
}

int rt_present_scaled(rt_ctx* c, int out_width, int out_height, int top_down) {
  if (!c || !scaled_size_ok(out_width, out_height)) return RT_E_INVAL;
  if (!whole_frame(c)) return RT_E_STATE;
  RT_HIP(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)rt_image_stream(c);  // as rt_present: after the image's writer, before the next
  const size_t bytes = (size_t)out_width * out_height * 4;
  unsigned char* dst = c->d_scaled_bound;
  if (!dst) {
    if (c->scaled_own_bytes < bytes) {
      if (c->d_scaled_own) {
        // a larger window: scaled presents already enqueued still write the old buffer, each on
        // one of the context's streams, so all of them are waited for before it is freed
        int rc = drain(c);
        if (rc != RT_OK) return rc;
        if (c->d_scaled == c->d_scaled_own) c->d_scaled = nullptr;
        RT_HIP(c, hipFree(c->d_scaled_own));
        c->d_scaled_own = nullptr;
        c->scaled_own_bytes = 0;
        st = (hipStream_t)rt_image_stream(c);
      }
      int rc = rt::alloc_or_nomem(&c->d_scaled_own, bytes, c->last_hip);
      if (rc != RT_OK) return rc;
      c->scaled_own_bytes = bytes;
      RT_HIP(c, hipMemsetAsync(c->d_scaled_own, 0, bytes, st));
    }
    dst = c->d_scaled_own;
  }
  RT_HIP(c, rt::launch_present_scaled(c->d_image, c->cfg.width, c->cfg.height, dst, out_width, out_height,
                                      top_down != 0, st, c->log));
  c->d_scaled = dst;
  c->scaled_w = out_width;
  c->scaled_h = out_height;
  return RT_OK;
}

void* rt_present_scaled_device_ptr(rt_ctx* c) { return c ? (void*)c->d_scaled : nullptr; }

int rt_present_scaled_size(rt_ctx* c, int* out_width, int* out_height) {
  if (!c) return RT_E_INVAL;
  if (!whole_frame(c) || !c->d_scaled) return RT_E_STATE;
  if (out_width) *out_width = c->scaled_w;
  if (out_height) *out_height = c->scaled_h;
  return RT_OK;
}

int rt_bind_present_scaled(rt_ctx* c, void* p) {
  if (!c || ((uintptr_t)p & 3)) return RT_E_INVAL;  // the kernel stores whole pixels
  if (!whole_frame(c)) return RT_E_STATE;
  c->d_scaled_bound = (unsigned char*)p;
  return RT_OK;
}

int rt_download_rgba8_scaled(rt_ctx* c, int out_width, int out_height, int top_down, uint8_t* out) {
  if (!c || !out) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int rc = rt_present_scaled(c, out_width, out_height, top_down);
  if (rc == RT_OK) rc = drain(c);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipMemcpyAsync(out, c->d_scaled, (size_t)out_width * out_height * 4, hipMemcpyDeviceToHost, c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---- ray queries (include/rt/abi.h "Ray queries") -------------------------------------------
// the scene in effect: the table and camera of the header last given to the context
static rt::QueryScene query_scene(const rt_ctx* c) {
  rt::QueryScene s{};
  s.shapes = c->d_scene;
  s.S = table_stride(c);
  s.nobj = c->nobj;
  s.nplanes = c->nplanes;
  s.nrects = c->nrects;
  s.fW = (float)c->cfg.width;
  s.fH = (float)c->cfg.height;
  const float *h = hv(c, RT_HDR_HORIZONTAL), *v = hv(c, RT_HDR_VERTICAL), *l = hv(c, RT_HDR_LLC_MINUS_CAMPOS),
              *cam = hv(c, RT_HDR_CAMERA_LOCATION);
  s.hx = h[0]; s.hy = h[1]; s.hz = h[2];
  s.vx = v[0]; s.vy = v[1]; s.vz = v[2];
  s.lx = l[0]; s.ly = l[1]; s.lz = l[2];
  s.cx = cam[0]; s.cy = cam[1]; s.cz = cam[2];
  return s;
}
// the scene's query tree as a launch argument (v: where it is built), null when off or not built
static const rt::QueryTree* query_tree(const rt_ctx* c, rt::QueryTree& v) { return c->tree.view(v); }
static bool query_thr_ok(float thr) { return thr >= 0.0f && thr <= 3.402823466e+38f; }  // finite and >= 0; NaN fails
// The checks every query starts with, then the main stream ordered behind everything the context
// has enqueued (the pipelined streams joined with the context's own events: nothing is created).
// RT_OK: go on; 1: nothing to do (n == 0); else the status to return.
static int query_begin(rt_ctx* c, size_t n, bool inputs) {
  if (!c || n > RT_QUERY_MAX_RAYS) return RT_E_INVAL;
  if (!c->have_header) return RT_E_STATE;
  if (n == 0) return 1;
  if (!inputs) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  return join(c);
}
#define RT_QUERY_BEGIN(c, n, inputs)         \
  do {                                       \
    const int _rc = query_begin(c, n, inputs); \
    if (_rc != RT_OK) return _rc < 0 ? _rc : RT_OK; \
  } while (0)

int rt_trace_rays(rt_ctx* c, const float* origins, const float* dirs, size_t n, float thr, float* t, int32_t* ind,
                  float* normals) {
  if (!query_thr_ok(thr)) return RT_E_INVAL;
  RT_QUERY_BEGIN(c, n, origins && dirs);
  rt::QueryTree tv{};
  return c->query.trace(query_scene(c), query_tree(c, tv), origins, dirs, nullptr, n, thr, t, ind, normals, nullptr, c->stream, c->last_hip);
}

int rt_trace_pixels(rt_ctx* c, const int32_t* xy, size_t n, float thr, float* t, int32_t* ind, float* normals,
                    float* dirs) {
  if (!query_thr_ok(thr)) return RT_E_INVAL;
  RT_QUERY_BEGIN(c, n, xy != nullptr);
  rt::QueryTree tv{};
  return c->query.trace(query_scene(c), query_tree(c, tv), nullptr, nullptr, xy, n, thr, t, ind, normals, dirs, c->stream, c->last_hip);
}

int rt_occluded(rt_ctx* c, const float* from, const float* to, size_t n, uint8_t* out) {
  RT_QUERY_BEGIN(c, n, from && to);
  rt::QueryTree tv{};
  if (!out) return RT_OK;
  return c->query.occluded(query_scene(c), query_tree(c, tv), from, to, n, out, c->stream, c->last_hip);
}

int rt_trace_rays_device(rt_ctx* c, const void* d_origins, const void* d_dirs, size_t n, float thr, void* d_t,
                         void* d_ind, void* d_normals) {
  if (!query_thr_ok(thr)) return RT_E_INVAL;
  RT_QUERY_BEGIN(c, n, d_origins && d_dirs);
  rt::QueryTree tv{};
  rt::RayQuery q{};
  q.sc = query_scene(c);
  q.origins = (const float*)d_origins;
  q.dirs = (const float*)d_dirs;
  q.n = n;
  q.thr = thr;
  q.t = (float*)d_t;
  q.ind = (int*)d_ind;
  q.nrm = (float*)d_normals;
  RT_HIP(c, rt::launch_ray_query(q, c->stream, query_tree(c, tv), c->log));
  return RT_OK;
}

int rt_trace_pixels_device(rt_ctx* c, const void* d_xy, size_t n, float thr, void* d_t, void* d_ind, void* d_normals,
                           void* d_dirs) {
  if (!query_thr_ok(thr)) return RT_E_INVAL;
  RT_QUERY_BEGIN(c, n, d_xy != nullptr);
  rt::QueryTree tv{};
  rt::RayQuery q{};
  q.sc = query_scene(c);
  q.xy = (const int*)d_xy;
  q.n = n;
  q.thr = thr;
  q.t = (float*)d_t;
  q.ind = (int*)d_ind;
  q.nrm = (float*)d_normals;
  q.dir_out = (float*)d_dirs;
  RT_HIP(c, rt::launch_ray_query(q, c->stream, query_tree(c, tv), c->log));
  return RT_OK;
}

int rt_occluded_device(rt_ctx* c, const void* d_from, const void* d_to, size_t n, void* d_out) {
  RT_QUERY_BEGIN(c, n, d_from && d_to);
  rt::QueryTree tv{};
  if (!d_out) return RT_OK;
  RT_HIP(c, rt::launch_occluded(query_scene(c), (const float*)d_from, (const float*)d_to, n, (unsigned char*)d_out,
                                c->stream, query_tree(c, tv), c->log));
  return RT_OK;
}

size_t rt_query_workspace_bytes(rt_ctx* c) { return c ? c->query.bytes : 0; }

// ---- host-buffer parity path -----------------------------------------------------------
// the SSBO's pixel, normals and depth arrays (whole-frame contexts)
struct SsboArrays {
  float *pixels, *normals, *depth;
};
static SsboArrays ssbo_arrays(const rt_ctx* c, void* ssbo) {
  float* f = (float*)ssbo;
  const int S = c->cfg.num_shapes, A = c->cfg.spp, W = c->cfg.width, H = c->cfg.height, F = c->cfg.num_frames;
  return {f + rt_off_pixels(S, A) / 4, f + rt_off_normals(S, A, W, H, F) / 4, f + rt_off_depth(S, A, W, H, F) / 4};
}

static int hostbuf_in(rt_ctx* c, void* ssbo, int frame_num) {
  if (!c || !ssbo) return RT_E_INVAL;
  if (c->own0 != 0 || c->own_rows != c->cfg.height) return RT_E_STATE;  // whole-frame contexts only
  if (frame_num < 0 || frame_num >= c->cfg.num_frames) return RT_E_INVAL;
  ((float*)ssbo)[RT_HDR_MODE * 4 + 1] = (float)frame_num;  // ssbo_CPUMEM.mode.y = frame_num (main.cpp:584)
  int rc = rt_upload_header(c, ssbo, rt_header_bytes(c->cfg.num_shapes, c->cfg.spp));
  if (rc != RT_OK) return rc;
  const SsboArrays a = ssbo_arrays(c, ssbo);
  return rt_upload_gbuffer(c, a.pixels, a.normals, a.depth);
}

static int hostbuf_out(rt_ctx* c, void* ssbo, float* image) {
  const SsboArrays a = ssbo_arrays(c, ssbo);
  return rt_download(c, a.pixels, a.normals, a.depth, image);
}

int rt_compute_one_shader(rt_ctx* c, void* ssbo, int frame_num, int program, float* image) {
  int rc = hostbuf_in(c, ssbo, frame_num);
  if (rc != RT_OK) return rc;
  rc = run_program(c, program, frame_num);
  if (rc != RT_OK) return rc;
  rc = hostbuf_out(c, ssbo, image);
  if (rc != RT_OK) return rc;
  return (frame_num + 1) % c->cfg.num_frames;
}

int rt_compute_two_shaders(rt_ctx* c, void* ssbo, int frame_num, int p1, int p2, float* image) {
  int rc = hostbuf_in(c, ssbo, frame_num);
  if (rc != RT_OK) return rc;
  rc = run_program(c, p1, frame_num);
  if (rc == RT_OK) rc = run_program(c, p2, frame_num);
  if (rc != RT_OK) return rc;
  rc = hostbuf_out(c, ssbo, image);
  if (rc != RT_OK) return rc;
  return (frame_num + 1) % c->cfg.num_frames;
}

// ---- instrumentation ------------------------------------------------------------------
int rt_enable_timing(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  c->timing.on = on != 0;
  return RT_OK;
}

int rt_kernel_stats(rt_ctx* c, int program, int* launches, double* total_ms) {
  if (!c || program <= 0 || program >= RT_PROG_COUNT) return RT_E_INVAL;
  int rc = resolve_timing(c);
  if (rc != RT_OK) return rc;
  if (launches) *launches = c->timing.launches[program];
  if (total_ms) *total_ms = c->timing.total_ms[program];
  return RT_OK;
}

int rt_host_stats(rt_ctx* c, double* wait_ms, long long* waits) {
  if (!c) return RT_E_INVAL;
  if (wait_ms) *wait_ms = c->stage.wait_ms;
  if (waits) *waits = c->stage.waits;
  return RT_OK;
}

int rt_reset_stats(rt_ctx* c) {
  if (!c) return RT_E_INVAL;
  int rc = resolve_timing(c);
  if (rc != RT_OK) return rc;
  c->stage.reset_stats();
  c->timing.reset();
  return RT_OK;
}

int rt_enable_counters(rt_ctx* c, int on) {
  if (!c) return RT_E_INVAL;
  RT_HIP(c, hipSetDevice(c->device));
  int jr = join(c);
  if (jr != RT_OK) return jr;
  if (on && !c->d_counters) {
    RT_HIP(c, hipMalloc(&c->d_counters, rt::kCounters * rt::kCounterSlots * sizeof(unsigned long long)));
    RT_HIP(c, hipMemsetAsync(c->d_counters, 0, rt::kCounters * rt::kCounterSlots * sizeof(unsigned long long),
                             c->stream));
    RT_HIP(c, hipMalloc(&c->d_row_counters, (size_t)c->band_rows * sizeof(unsigned long long)));
    RT_HIP(c, hipMemsetAsync(c->d_row_counters, 0, (size_t)c->band_rows * sizeof(unsigned long long), c->stream));
  }
  c->counting = (on & 1) != 0;
  c->row_counting = (on & 2) != 0;
  return RT_OK;
}

int rt_read_counters(rt_ctx* c, uint64_t out[8], int reset) {
  if (!c || !out) return RT_E_INVAL;
  if (!c->d_counters) {
    for (int k = 0; k < rt::kCounters; ++k) out[k] = 0;
    return RT_OK;
  }
  RT_HIP(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h((size_t)rt::kCounters * rt::kCounterSlots);
  int rc = sync_all(c);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipMemcpy(h.data(), c->d_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < rt::kCounters; ++k) {
    unsigned long long sum = 0;
    for (int j = 0; j < rt::kCounterSlots; ++j) sum += h[(size_t)k * rt::kCounterSlots + j];
    out[k] = (uint64_t)sum;
  }
  if (reset) RT_HIP(c, hipMemset(c->d_counters, 0, h.size() * sizeof(unsigned long long)));
  return RT_OK;
}

int rt_read_row_counters(rt_ctx* c, uint64_t* rows, int reset) {
  if (!c || !rows) return RT_E_INVAL;
  const int R = c->own_rows;
  if (!c->d_row_counters) {
    for (int k = 0; k < R; ++k) rows[k] = 0;
    return RT_OK;
  }
  RT_HIP(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h(c->band_rows);
  int rc = sync_all(c);
  if (rc != RT_OK) return rc;
  RT_HIP(c, hipMemcpy(h.data(), c->d_row_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < R; ++k) rows[k] = (uint64_t)h[(size_t)(c->own0 - c->band0) + k];
  if (reset) RT_HIP(c, hipMemset(c->d_row_counters, 0, h.size() * sizeof(unsigned long long)));
  return RT_OK;
}

int rt_selftest_math(rt_ctx* c, int fn, const float* in, float* out, size_t n) {
  if (!c || !in || !out || fn < 0 || fn > RT_MATH_CULL_TREE) return RT_E_INVAL;
  // RT_MATH_CULL_CLUSTER's wave-mask form needs full waves; RT_MATH_CULL_TREE takes its cases, under the same rule
  if ((fn == RT_MATH_CULL_CLUSTER || fn == RT_MATH_CULL_TREE) && n % 64 != 0) return RT_E_INVAL;
  static const int in_w[] = {1, 2, 1, 2, 3, 10, 0, 0, 0, 0, 4, 0, 24, 28, 452, 14, 263, 14},
                   out_w[] = {1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 5, 2, 7, 2, 320, 3, 128, 3};
  RT_HIP(c, hipSetDevice(c->device));
  float *din = nullptr, *dout = nullptr;
  const bool sweep = fn == RT_MATH_SQRT_SWEEP || fn == RT_MATH_RCP_SWEEP || fn == RT_MATH_SQRT_TAIL_SWEEP ||
                     fn == RT_MATH_SIN_RANGE || fn == RT_MATH_SIN_TABLE;  // in: one float (the count or the first bit pattern)
  size_t ib = sweep ? sizeof(float) : n * in_w[fn] * sizeof(float);
  size_t ob = n * out_w[fn] * sizeof(float);
  RT_HIP(c, hipMalloc(&din, std::max<size_t>(ib, 4)));
  hipError_t e = hipMalloc(&dout, std::max<size_t>(ob, 4));
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = rt::launch_selftest(fn, din, dout, n, c->stream, c->log);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  if (e != hipSuccess) return hip_fail(c, e);
  return RT_OK;
}

}  // extern "C"
