// rt_cull.h — the cull cache: the AO pools' primary-ray cull masks while camera and scene hold.
#pragma once
#include <vector>

#include "rt_hip_util.h"
#include "rt_kernels.h"

namespace rt {

// Cull cache.  The AO kernel's pool start culls the sphere table against the cone of the pool's
// primary rays; its inputs are the camera, the frame and strip geometry, spp, nobj and the sphere
// rows (rt_plan cull_key), none of which the render loop's per-frame update touches (it replaces
// rand_buffer and mode.y).  While the key holds, the pools' masks are kept in a device table
// (rt::launch_cull_fill) and the AO launches load them (FrameParams::cull):
//  - a launch whose key differs from the previous launch's runs the in-kernel cull and marks the
//    table invalid; so does the first launch that repeats a key (a camera that rests for one
//    frame pays nothing);
//  - the second launch in a row that repeats the key enqueues the fill on its own stream, before
//    itself, when the table is invalid; it and its successors load the masks.
// Nothing waits on the host.  Pipelined AO passes alternate between streams: a stream's first
// cached launch after a fill waits for the fill's event, and a refill waits for the events of
// the last cached launches on every stream (recorded when the table was marked invalid).
// Sort frames.  The fill also traces each pool's unjittered centre ray and keeps two unit vectors
// orthogonal to the surface normal at its hit: 32 bytes per pool in front of the masks, in the same
// allocation, so they share the masks' key, fill, events and invalidation.  The sorted cached
// kernels deal a pool's samples by their sector around that normal (FrameParams::cull_frames).
// When masks and frames together exceed the cap, or their allocation fails and the masks' alone
// succeeds, the context keeps the masks only and the kernels their octant key.
// Tables above kCullCacheMaxBytes are never built: those contexts, scenes with planes, and contexts
// whose allocation failed keep the in-kernel cull.  The cap admits config (e)'s 265 MB (7680x4320,
// 64 spp, 256 spheres: 8.3 M pools of 4 words, 1.5% of what that context's g-buffer ring holds),
// whose launches gain 2% from it (DESIGN.md §5 "Round 9").
#ifndef RT_CULL_CACHE_MAX_MB
#define RT_CULL_CACHE_MAX_MB 512  // (A/B builds override it)
#endif
constexpr size_t kCullCacheMaxBytes = (size_t)RT_CULL_CACHE_MAX_MB << 20;
constexpr int kCullRepeats = 2;  // launches in a row that must repeat a key before the table is filled
struct CullCache {
  bool on = true;                    // rt_set_cull_cache
  bool nomem = false;                // the allocation failed once: never cached
  size_t cap = kCullCacheMaxBytes;   // rt_debug_cull_cache_cap (test hook): this context's cap
  void* d_alloc = nullptr;           // the allocation: frame_bytes of sort frames, then d_table
  size_t frame_bytes = 0;            // 0: masks only
  unsigned long long* d_table = nullptr;
  size_t bytes = 0;                  // of d_table: pools x ceil(num_shapes / 64) words
  std::vector<unsigned char> key;    // the previous eligible launch's key
  std::vector<unsigned char> next;   // scratch: the key of the launch being made
  bool have_key = false;
  int repeats = 0;                   // launches in a row that repeated `key`
  bool valid = false;                // d_table holds `key`'s masks
  hipEvent_t ev_fill = nullptr;
  StreamSet seen;                    // streams ordered after the fill
  StreamSet readers;                 // streams with cached launches since the fill
  hipEvent_t ev_read[kAoStreams] = {};   // the last cached launches, one per reader stream
  int n_read = 0;                    // ev_read[0 .. n_read) are recorded and not yet waited for
  long long fills = 0, cached = 0;   // rt_cull_cache_stats
  LaunchLog* log = nullptr;          // the context's launch log while it is on (rt_debug_launch_log)
  // Pool list (rt_kernels.h ao_pool_list_bytes): the non-sky pools' (pb, xf, yf, np) rows and the
  // sky pools' indices, in front of the frames in the same allocation when masks, frames and list
  // fit the cap together.  Written on the fill's stream right after the fill; its two counts are
  // copied to pinned memory behind it and ev_list recorded.  The launches poll that event and never
  // wait for it: until it has fired they run the cached kernel over every pool, from then on over
  // the list's blocks (FrameParams::cull_frames == 2).  Key, allocation, ev_fill / ev_read and
  // invalidation are the masks'.
  bool list_on = true;               // rt_set_pool_list
  size_t list_bytes = 0;             // 0: no list in this allocation
  long long list_pools = 0;          // the pools the list was laid out for
  int* h_counts = nullptr;           // pinned: (n_nonsky, n_sky, 0, 0)
  hipEvent_t ev_list = nullptr;
  bool list_pending = false;         // written for the current fill; ev_list has not been seen fired
  bool list_ready = false;           // h_counts holds the current fill's counts
  long long list_builds = 0, list_launches = 0;  // rt_pool_list_stats

  // Before an AO launch of p (its rows, tables and camera set) on st, of a context with
  // configuration cfg and header h: compare its key with the previous launch's and hand it the
  // table (p.cull) when the key has held, after filling the table if it is invalid.
  int before(const rt_config& cfg, const float* h, FrameParams& p, hipStream_t st, int& last_hip);
  // the table is no longer the current key's: the cached launches enqueued so far are its last readers
  int invalidate(int& last_hip);
  // every stream has been drained: nothing in flight reads or writes the table
  void streams_idle();
  void release();
};

}  // namespace rt
