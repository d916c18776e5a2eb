// rt_gbuf.h — the g-buffer ring: per-slot device arrays of pixels, normals and depth, each reached
// through a slot -> buffer map, with the buffers outside the maps that pipelined mode 1 rotates.
#pragma once
#include <utility>
#include <vector>

#include "rt_hip_util.h"
#include "rt_kernels.h"

namespace rt {

// Pipelining depth D: AO k waits for post k-D, the last reader of the raw pixel buffer and the
// normals/depth buffers it overwrites (D of each rotate outside the slot map)
constexpr int kPipe = 4;  // capacity; the depth in use is the context's pipe_depth (default 3)

// Slot layouts on the device (rt_kernels_impl.h): pixels are [band_rows][W] float4; normals are
// a [band_rows][W] xyz plane (12 B) then a w plane (4 B) (nrm_store); depth is two [band_rows][W]
// float2 planes, (x, y) then (z, w) (dep_store).
enum SlotKind { kPixels = 0, kNormals = 1, kDepth = 2, kSlotKinds = 3 };

struct SlotRing {
  std::vector<float4*> buf;  // F + depth buffers
  std::vector<int> slot;     // slot -> buffer index
  float4* at(int s) const { return buf[slot[s]]; }
};

struct GbufRing {
  SlotRing ring[kSlotKinds];  // by SlotKind
  int spare = 0;              // pixel buffer outside the map (sequential post-process target)
  int raw_buf[kPipe] = {};    // raw_buf[1..]: more pixel buffers outside the map (pipelined raw AO output)
  int nrm_free[kPipe] = {}, dep_free[kPipe] = {};  // buffers outside the maps, oldest first

  // F slots and `depth` more buffers of each kind, slot_bytes each, zeroed on st (value-initialised
  // ssbo_CPUMEM: the ring starts at zero)
  hipError_t create(int F, int depth, size_t slot_bytes, hipStream_t st);
  void release();

  float4* pixels(int s) const { return ring[kPixels].at(s); }
  // the history of every slot, and slot `frame`'s normals / depth as the launch's own
  void fill(FrameParams& p, int F, int frame) const;
  // sequential post-process: filtered out of place into the spare, which then becomes slot `frame`
  float4* spare_pixels() const { return ring[kPixels].buf[spare]; }
  void swap_spare(int frame) { std::swap(ring[kPixels].slot[frame], spare); }
  // pipelined frame number nq (mod D): its raw pixel buffer (the sequential spare is raw buffer 0)
  float4* raw(int nq) const { return ring[kPixels].buf[nq == 0 ? spare : raw_buf[nq]]; }
  // pipelined AO writes into the oldest free normals / depth buffers (p.nrm / p.dep; the slot's
  // previous contents stay p.nrm_prev / p.dep_prev) ...
  void fresh(FrameParams& p) const;
  // ... which slot `frame` then maps to; its previous ones join the back of the free queues of D
  void rotate(int frame, int D);
};

}  // namespace rt
