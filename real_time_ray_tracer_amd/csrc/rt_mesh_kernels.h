// rt_mesh_kernels.h — the mesh queries' launches (rt_mesh_kernels.hip) as rt_mesh.hip calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {
namespace mesh {

// the uploaded hierarchy: nodes [n_nodes][2] float4 (lo.xyz | skip, hi.xyz | first * 16 + count),
// tris [n_entries][3] float4 in leaf order (v0.xyz | index, v1.xyz, v2.xyz); rt_mesh_host.h pack_tables
struct MeshView {
  const float4* nodes;
  const float4* tris;
  int n_nodes;
  int n_entries;
};

struct MeshTrace {
  MeshView m;
  const float* origins;  // [n][3], or [3] with RT_MESH_ONE_ORIGIN
  const float* dirs;     // [n][3]
  size_t n;
  int flags;
  float thr;
  float* t;    // outputs, any of them NULL; with RT_MESH_MERGE t is in-out and not NULL
  int* prim;
  float* nrm;
  float* uv;
};

constexpr int kMeshBlock = 256;

hipError_t launch_mesh_trace(const MeshTrace& q, hipStream_t stream);
hipError_t launch_mesh_occluded(const MeshView& m, const float* from, const float* to, size_t n, int flags,
                                unsigned char* out, hipStream_t stream);

}  // namespace mesh
}  // namespace rt
