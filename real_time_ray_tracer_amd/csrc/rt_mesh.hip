// rt_mesh.hip — the rt_mesh object of librtrt_mesh.so (include/rt/mesh.h): the hierarchy built on
// the host (rt_mesh_host.cpp) and uploaded once, the host-pointer queries' workspace, the launches.
#include <new>
#include <vector>

#include "../../include/rt/mesh.h"
#include "rt_hip_util.h"
#include "rt_mesh_host.h"
#include "rt_mesh_kernels.h"

struct rt_mesh {
  int device = 0;
  int last_hip = 0;
  hipStream_t stream = nullptr;  // the mesh's own
  float4* d_nodes = nullptr;
  float4* d_tris = nullptr;
  rt::mesh::MeshView view{};
  int leaves = 0, dead = 0;
  size_t bytes = 0;
  unsigned char* d_work = nullptr;  // the host-pointer queries' workspace: grows, never shrinks
  size_t work_bytes = 0;
};

namespace {

using rt::alloc_or_nomem;
using rt::hip_fail;

// the workspace's parts start on 256-byte boundaries
constexpr size_t kPart = 256;
size_t part(size_t bytes) { return (bytes + kPart - 1) / kPart * kPart; }

bool thr_ok(float thr) { return thr >= 0.0f && thr <= 3.402823466e+38f; }

int reserve(rt_mesh* m, size_t need) {
  if (need <= m->work_bytes) return RT_OK;
  if (m->d_work) {
    RT_HIP(m->last_hip, hipFree(m->d_work));
    m->d_work = nullptr;
    m->work_bytes = 0;
  }
  int rc = alloc_or_nomem(&m->d_work, need, m->last_hip);
  if (rc != RT_OK) return rc;
  m->work_bytes = need;
  return RT_OK;
}

void release(rt_mesh* m) {
  if (m->d_work) (void)hipFree(m->d_work);
  if (m->d_nodes) (void)hipFree(m->d_nodes);
  if (m->d_tris) (void)hipFree(m->d_tris);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

int upload(rt_mesh* m, const float* verts, const int32_t* tris, int nt) {
  rt::mesh::Bvh b;
  rt::mesh::build_bvh(verts, tris, nt, b);
  if (!rt::mesh::bvh_valid(b)) return RT_E_STATE;  // (never: the build's own output)
  std::vector<float> nodes, leaf_tris;
  rt::mesh::pack_tables(verts, tris, b, nodes, leaf_tris);
  RT_HIP(m->last_hip, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  // (an empty table still gets a buffer: the kernels' pointers are never NULL)
  const size_t nb = nodes.size() * sizeof(float), tb = leaf_tris.size() * sizeof(float);
  int rc = alloc_or_nomem(&m->d_nodes, nb ? nb : 32, m->last_hip);
  if (rc != RT_OK) return rc;
  rc = alloc_or_nomem(&m->d_tris, tb ? tb : 48, m->last_hip);
  if (rc != RT_OK) return rc;
  if (nb) RT_HIP(m->last_hip, hipMemcpy(m->d_nodes, nodes.data(), nb, hipMemcpyHostToDevice));
  if (tb) RT_HIP(m->last_hip, hipMemcpy(m->d_tris, leaf_tris.data(), tb, hipMemcpyHostToDevice));
  m->view = rt::mesh::MeshView{m->d_nodes, m->d_tris, b.nodes, (int)b.order.size()};
  m->leaves = b.leaves;
  m->dead = b.dead;
  m->bytes = nb + tb;
  return RT_OK;
}

int check_trace(const rt_mesh* m, const void* origins, const void* dirs, size_t n, int flags, float thr, const void* t) {
  if (!m || (flags & ~(RT_MESH_ONE_ORIGIN | RT_MESH_MERGE)) != 0 || n > RT_QUERY_MAX_RAYS || !thr_ok(thr)) return RT_E_INVAL;
  if (n > 0 && (!origins || !dirs || ((flags & RT_MESH_MERGE) && !t))) return RT_E_INVAL;
  return RT_OK;
}

int check_occluded(const rt_mesh* m, const void* from, const void* to, size_t n, int flags, const void* out) {
  if (!m || (flags & ~RT_MESH_MERGE) != 0 || n > RT_QUERY_MAX_RAYS) return RT_E_INVAL;
  if (n > 0 && (!from || !to || ((flags & RT_MESH_MERGE) && !out))) return RT_E_INVAL;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_mesh_create(int device, const float* verts, int nv, const int32_t* tris, int nt, rt_mesh** out) {
  if (!out) return RT_E_INVAL;
  *out = nullptr;
  int rc = rt::mesh::check_mesh(verts, nv, tris, nt);
  if (rc != RT_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return RT_E_NODEV;
  }
  if (device < 0 || device >= ndev) return RT_E_NODEV;
  rt_mesh* m = new (std::nothrow) rt_mesh;
  if (!m) return RT_E_NOMEM;
  m->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete m;
    return RT_E_NODEV;
  }
  rc = upload(m, verts, tris, nt);
  if (rc != RT_OK) {
    release(m);
    return rc;
  }
  *out = m;
  return RT_OK;
}

int rt_mesh_destroy(rt_mesh* m) {
  if (!m) return RT_E_INVAL;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  release(m);
  return RT_OK;
}

int rt_mesh_stats(const rt_mesh* m, int* nodes, int* leaves, int* dead, size_t* bytes) {
  if (!m) return RT_E_INVAL;
  if (nodes) *nodes = m->view.n_nodes;
  if (leaves) *leaves = m->leaves;
  if (dead) *dead = m->dead;
  if (bytes) *bytes = m->bytes;
  return RT_OK;
}

int rt_mesh_last_hip_error(const rt_mesh* m) { return m ? m->last_hip : 0; }

size_t rt_mesh_workspace_bytes(const rt_mesh* m) { return m ? m->work_bytes : 0; }

int rt_mesh_synchronize(rt_mesh* m) {
  if (!m) return RT_E_INVAL;
  RT_HIP(m->last_hip, hipSetDevice(m->device));
  RT_HIP(m->last_hip, hipStreamSynchronize(m->stream));
  return RT_OK;
}

int rt_mesh_trace_rays_device(rt_mesh* m, void* hip_stream, const float* d_origins, const float* d_dirs, size_t n,
                              int flags, float thr, float* d_t, int32_t* d_prim, float* d_normals, float* d_uv) {
  int rc = check_trace(m, d_origins, d_dirs, n, flags, thr, d_t);
  if (rc != RT_OK || n == 0) return rc;
  RT_HIP(m->last_hip, hipSetDevice(m->device));
  const rt::mesh::MeshTrace q{m->view, d_origins, d_dirs, n, flags, thr, d_t, d_prim, d_normals, d_uv};
  RT_HIP(m->last_hip, rt::mesh::launch_mesh_trace(q, hip_stream ? (hipStream_t)hip_stream : m->stream));
  return RT_OK;
}

int rt_mesh_occluded_device(rt_mesh* m, void* hip_stream, const float* d_from, const float* d_to, size_t n, int flags,
                            uint8_t* d_out) {
  int rc = check_occluded(m, d_from, d_to, n, flags, d_out);
  if (rc != RT_OK || n == 0 || !d_out) return rc;
  RT_HIP(m->last_hip, hipSetDevice(m->device));
  RT_HIP(m->last_hip, rt::mesh::launch_mesh_occluded(m->view, d_from, d_to, n, flags, d_out,
                                                     hip_stream ? (hipStream_t)hip_stream : m->stream));
  return RT_OK;
}

int rt_mesh_trace_rays(rt_mesh* m, const float* origins, const float* dirs, size_t n, int flags, float thr, float* t,
                       int32_t* prim, float* normals, float* uv) {
  int rc = check_trace(m, origins, dirs, n, flags, thr, t);
  if (rc != RT_OK || n == 0) return rc;
  RT_HIP(m->last_hip, hipSetDevice(m->device));
  const bool merge = (flags & RT_MESH_MERGE) != 0;
  const size_t v3 = part(n * 3 * sizeof(float)), v2 = part(n * 2 * sizeof(float)), v1 = part(n * sizeof(float));
  const size_t o_bytes = (flags & RT_MESH_ONE_ORIGIN) ? 3 * sizeof(float) : n * 3 * sizeof(float);
  // inputs: origins | dirs;  outputs: t | prim | normals | uv (each only when asked for)
  rc = reserve(m, part(o_bytes) + v3 + (t ? v1 : 0) + (prim ? v1 : 0) + (normals ? v3 : 0) + (uv ? v2 : 0));
  if (rc != RT_OK) return rc;
  hipStream_t st = m->stream;
  unsigned char* p = m->d_work;
  rt::mesh::MeshTrace q{m->view, (const float*)p, (const float*)(p + part(o_bytes)), n, flags, thr, nullptr, nullptr, nullptr, nullptr};
  RT_HIP(m->last_hip, hipMemcpyAsync(p, origins, o_bytes, hipMemcpyHostToDevice, st));
  RT_HIP(m->last_hip, hipMemcpyAsync(p + part(o_bytes), dirs, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  p += part(o_bytes) + v3;
  if (t) q.t = (float*)p, p += v1;
  if (prim) q.prim = (int*)p, p += v1;
  if (normals) q.nrm = (float*)p, p += v3;
  if (uv) q.uv = (float*)p, p += v2;
  if (merge) {  // the earlier answer goes in
    RT_HIP(m->last_hip, hipMemcpyAsync(q.t, t, n * sizeof(float), hipMemcpyHostToDevice, st));
    if (normals) RT_HIP(m->last_hip, hipMemcpyAsync(q.nrm, normals, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  }
  RT_HIP(m->last_hip, rt::mesh::launch_mesh_trace(q, st));
  if (t) RT_HIP(m->last_hip, hipMemcpyAsync(t, q.t, n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (prim) RT_HIP(m->last_hip, hipMemcpyAsync(prim, q.prim, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (normals) RT_HIP(m->last_hip, hipMemcpyAsync(normals, q.nrm, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (uv) RT_HIP(m->last_hip, hipMemcpyAsync(uv, q.uv, n * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
  RT_HIP(m->last_hip, hipStreamSynchronize(st));
  return RT_OK;
}

int rt_mesh_occluded(rt_mesh* m, const float* from, const float* to, size_t n, int flags, uint8_t* out) {
  int rc = check_occluded(m, from, to, n, flags, out);
  if (rc != RT_OK || n == 0 || !out) return rc;
  RT_HIP(m->last_hip, hipSetDevice(m->device));
  const size_t v3 = part(n * 3 * sizeof(float));
  rc = reserve(m, 2 * v3 + part(n));
  if (rc != RT_OK) return rc;
  hipStream_t st = m->stream;
  unsigned char* p = m->d_work;
  RT_HIP(m->last_hip, hipMemcpyAsync(p, from, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  RT_HIP(m->last_hip, hipMemcpyAsync(p + v3, to, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  if (flags & RT_MESH_MERGE) RT_HIP(m->last_hip, hipMemcpyAsync(p + 2 * v3, out, n, hipMemcpyHostToDevice, st));
  RT_HIP(m->last_hip, rt::mesh::launch_mesh_occluded(m->view, (const float*)p, (const float*)(p + v3), n, flags, p + 2 * v3, st));
  RT_HIP(m->last_hip, hipMemcpyAsync(out, p + 2 * v3, n, hipMemcpyDeviceToHost, st));
  RT_HIP(m->last_hip, hipStreamSynchronize(st));
  return RT_OK;
}

}  // extern "C"
