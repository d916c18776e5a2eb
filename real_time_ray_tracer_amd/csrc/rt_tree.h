// rt_tree.h — the ray queries' tree on the device (include/rt/abi.h "Query tree"): the switch, the
// one device buffer, and the rebuild when the spheres change.  The tree itself is rt_plan's
// build_query_tree; the kernels that walk it are rt_kernels_impl.h's ray_query_tree_kernel and
// occluded_tree_kernel.
#pragma once
#include <vector>

#include "rt_hip_util.h"
#include "rt_kernels.h"
#include "rt_plan.h"
#include "rt_stage.h"

namespace rt {

// Off by default: a context that never switches it on allocates nothing, builds nothing and
// launches the linear kernels.  Switching on allocates d_buf once, for the largest tree that
// num_shapes rows can give; no later call allocates device memory for the tree.  While on, every
// call that gives the context a header calls update(), which rebuilds and uploads only when the
// bytes the tree depends on (nobj and the first nobj rows of the packed sphere table) differ from
// the last build's: a render loop that moves the light or replaces rand_buffer builds once.
struct QueryTreeState {
  bool on = false;
  unsigned char* d_buf = nullptr;  // nodes (two float4 each) | leaf and always rows | their indices
  size_t bytes = 0;                // of d_buf
  int cap = 0;                     // the num_shapes d_buf was sized for
  QueryTreeHost host;              // the last build
  int n_nodes = 0;                 // 0: no tree for the scene in effect (the linear kernels run)
  bool have_key = false;
  std::vector<unsigned char> key;    // nobj, then the sphere rows the last build read
  std::vector<unsigned char> image;  // scratch: the bytes of one upload
  long long builds = 0;

  // bytes of the buffer for a context of num_shapes shapes
  static size_t buffer_bytes(int num_shapes);
  // Allocate for num_shapes; the caller has made sure that no launch is in flight.
  int enable(int num_shapes, int& last_hip);
  // The sphere table of the header now in effect: rebuild if its bytes differ, upload through the
  // staging ring on st (the stream the queries run on, so a query enqueued before sees the old
  // tree and one enqueued after the new).  No allocation, no host wait beyond the ring's own.
  int update(const Row* sph, int nobj, StageRing& stage, hipStream_t st, int& last_hip);
  // The launch argument: null when off or when the scene has no tree.
  const QueryTree* view(QueryTree& v) const;
  // Off: frees the buffer; the caller has waited for the context's streams.
  void release();
};

}  // namespace rt
