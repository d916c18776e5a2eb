// rt_mesh_kernels.hip — the mesh queries on gfx950 (include/rt/mesh.h): one ray per lane walks the
// hierarchy's preorder node table over its skip links, without a stack, LDS or scratch, and tests a
// leaf's members with the rule's arithmetic (rt_mesh_rule.h) on the rule's operands: the leaf table
// holds each member's three vertices as they were given.  Nodes are 32 bytes, read as two 16-byte
// loads; a member is three.  Nothing is pruned by the closest t so far, so the answer is the
// brute-force loop's, bit for bit (mesh.h, "Why the gate is part of the rule").
//
// The walk ends and stays in bounds for any table: the node index strictly increases (the host
// checks skip > k before upload, and the walk takes at least k + 1 whatever it reads), and a member
// slot is compared against the table's length.  NaN and infinite rays never enter it.
#include "rt_mesh_kernels.h"

#include "../../include/rt/mesh.h"
#define RT_MESH_RULE_DEVICE
#include "rt_mesh_rule.h"

namespace rt {

using namespace mesh;

namespace {

__device__ __forceinline__ V3 xyz(float4 v) { return V3{v.x, v.y, v.z}; }
__device__ __forceinline__ V3 load3(const float* __restrict__ p, size_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// Calls f(slot, index, v0, v1, v2) for every member of every leaf whose box, and whose ancestors'
// boxes, the ray passes; f returns true to stop the walk.
template <class F>
__device__ __forceinline__ void walk(const MeshView& m, const Ray& r, F f) {
  const float4* __restrict__ nodes = m.nodes;
  const float4* __restrict__ tris = m.tris;
  const int nn = m.n_nodes;
  int k = 0;
  while (k < nn) {
    const float4 a = nodes[2 * (size_t)k], b = nodes[2 * (size_t)k + 1];
    int next = __float_as_int(a.w);
    if (box_pass(r, xyz(a), xyz(b))) {
      next = k + 1;
      const int fc = __float_as_int(b.w);
      const int first = fc >> 4, count = fc & 15;
      for (int j = 0; j < count; ++j) {
        const int slot = first + j;
        if (slot < 0 || slot >= m.n_entries) break;  // (never: the host checks the ranges)
        const float4 p0 = tris[3 * (size_t)slot], p1 = tris[3 * (size_t)slot + 1], p2 = tris[3 * (size_t)slot + 2];
        if (f(slot, __float_as_int(p0.w), xyz(p0), xyz(p1), xyz(p2))) return;
      }
    }
    k = next > k ? next : k + 1;
  }
}

}  // namespace

// Closest hit, one ray per lane: mesh.h's loop merged order-free by (t, index).
__global__ __launch_bounds__(kMeshBlock) void mesh_trace_kernel(MeshTrace Q) {
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= Q.n) return;
  const Ray r = make_ray(load3(Q.origins, (Q.flags & RT_MESH_ONE_ORIGIN) ? 0 : i), load3(Q.dirs, i));
  Hit best{-1.0f, 0.0f, 0.0f};
  int prim = -1, at = -1;
  const float thr = Q.thr;
  if (r.ok)
    walk(Q.m, r, [&](int slot, int index, V3 v0, V3 v1, V3 v2) {
      const Hit h = tri_eval(r, v0, v1, v2);
      if (closer(h.t, index, thr, best.t, prim)) {
        best = h;
        prim = index;
        at = slot;
      }
      return false;
    });
  if ((Q.flags & RT_MESH_MERGE) && !merge_takes(best.t, prim, Q.t[i])) {  // the existing answer stands
    if (Q.prim) Q.prim[i] = -1;
    if (Q.uv) Q.uv[2 * i] = 0.0f, Q.uv[2 * i + 1] = 0.0f;
    return;
  }
  if (Q.t) Q.t[i] = best.t;
  if (Q.prim) Q.prim[i] = prim;
  if (Q.nrm) {
    V3 n{0.0f, 0.0f, 0.0f};
    if (at >= 0) n = tri_normal(xyz(Q.m.tris[3 * (size_t)at]), xyz(Q.m.tris[3 * (size_t)at + 1]), xyz(Q.m.tris[3 * (size_t)at + 2]));
    Q.nrm[3 * i] = n.x;
    Q.nrm[3 * i + 1] = n.y;
    Q.nrm[3 * i + 2] = n.z;
  }
  if (Q.uv) Q.uv[2 * i] = best.u, Q.uv[2 * i + 1] = best.v;
}

// Occlusion, one segment per lane: rt_occluded's rule with tri_eval as eval_ray; the walk stops at
// the first occluder ("some occluder exists" does not depend on the order).
__global__ __launch_bounds__(kMeshBlock) void mesh_occluded_kernel(MeshView m, const float* __restrict__ from,
                                                                   const float* __restrict__ to, size_t n, int flags,
                                                                   unsigned char* out) {
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= n) return;
  float len;
  const Ray r = segment_ray(load3(from, i), load3(to, i), len);
  const double dlen = (double)len;
  bool occ = false;
  if (r.ok)
    walk(m, r, [&](int, int, V3 v0, V3 v1, V3 v2) {
      occ = occludes(tri_eval(r, v0, v1, v2).t, r.d, dlen);
      return occ;
    });
  const unsigned char mine = occ ? 1 : 0;
  out[i] = (flags & RT_MESH_MERGE) ? (unsigned char)((out[i] != 0) | mine) : mine;
}

namespace mesh {

hipError_t launch_mesh_trace(const MeshTrace& q, hipStream_t stream) {
  if (q.n == 0) return hipSuccess;
  const unsigned grid = (unsigned)((q.n + kMeshBlock - 1) / kMeshBlock);
  hipLaunchKernelGGL(mesh_trace_kernel, dim3(grid), dim3(kMeshBlock), 0, stream, q);
  return hipGetLastError();
}

hipError_t launch_mesh_occluded(const MeshView& m, const float* from, const float* to, size_t n, int flags,
                                unsigned char* out, hipStream_t stream) {
  if (n == 0 || !out) return hipSuccess;
  const unsigned grid = (unsigned)((n + kMeshBlock - 1) / kMeshBlock);
  hipLaunchKernelGGL(mesh_occluded_kernel, dim3(grid), dim3(kMeshBlock), 0, stream, m, from, to, n, flags, out);
  return hipGetLastError();
}

}  // namespace mesh
}  // namespace rt
