// rt_query.h — ray queries through host pointers: a device workspace of the context's own that
// stages the rays in and the answers out (include/rt/abi.h "Ray queries").  Allocated by the first
// query, replaced by one that needs more bytes, freed with the context; no allocation per call.
#pragma once
#include <stdint.h>

#include "rt_hip_util.h"
#include "rt_kernels.h"

namespace rt {

struct QueryWork {
  unsigned char* d_buf = nullptr;
  size_t bytes = 0;
  long long grows = 0;  // allocations so far (the first included)
  LaunchLog* log = nullptr;  // the context's launch log while it is on (rt_debug_launch_log)

  // Closest hits of n rays of scene sc on st: the rays copied in, the kernel, the answers copied out
  // into whichever outputs are non-null, and a wait for st.  xy non-null: pixel rays (origins and
  // dirs unused, dir_out the rays used); else the given rays.  tree: the scene's query tree, or null.
  int trace(const QueryScene& sc, const QueryTree* tree, const float* origins, const float* dirs, const int32_t* xy, size_t n, float thr,
            float* t, int32_t* ind, float* normals, float* dir_out, hipStream_t st, int& last_hip);
  // Occlusion of n segments, likewise.
  int occluded(const QueryScene& sc, const QueryTree* tree, const float* from, const float* to, size_t n, uint8_t* out, hipStream_t st,
               int& last_hip);
  void release();

 private:
  // at least `need` bytes; nothing is in flight on the old buffer (every query ends with a wait)
  int reserve(size_t need, int& last_hip);
};

}  // namespace rt
