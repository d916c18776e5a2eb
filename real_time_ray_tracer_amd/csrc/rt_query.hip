// rt_query.hip — the host-pointer ray queries' device workspace (rt_query.h).
#include "rt_query.h"

namespace rt {

namespace {

// the workspace's parts start on 256-byte boundaries
constexpr size_t kPart = 256;
size_t part(size_t bytes) { return (bytes + kPart - 1) / kPart * kPart; }

}  // namespace

int QueryWork::reserve(size_t need, int& last_hip) {
  if (need <= bytes) return RT_OK;
  if (d_buf) {
    RT_HIP(last_hip, hipFree(d_buf));
    d_buf = nullptr;
    bytes = 0;
  }
  int rc = alloc_or_nomem(&d_buf, need, last_hip);
  if (rc != RT_OK) return rc;
  bytes = need;
  ++grows;
  return RT_OK;
}

void QueryWork::release() {
  if (d_buf) (void)hipFree(d_buf);
  d_buf = nullptr;
  bytes = 0;
}

int QueryWork::trace(const QueryScene& sc, const QueryTree* tree, const float* origins, const float* dirs, const int32_t* xy, size_t n,
                     float thr, float* t, int32_t* ind, float* normals, float* dir_out, hipStream_t st, int& last_hip) {
  const size_t v3 = part(n * 3 * sizeof(float)), v1 = part(n * sizeof(float));
  // inputs: origins | dirs, or xy;  outputs: t | ind | normals | dir_out (each only when asked for)
  const size_t in_bytes = xy ? part(n * 2 * sizeof(int32_t)) : 2 * v3;
  const size_t need = in_bytes + (t ? v1 : 0) + (ind ? v1 : 0) + (normals ? v3 : 0) + (xy && dir_out ? v3 : 0);
  int rc = reserve(need, last_hip);
  if (rc != RT_OK) return rc;
  RayQuery q{};
  q.sc = sc;
  q.n = n;
  q.thr = thr;
  unsigned char* p = d_buf;
  if (xy) {
    q.xy = (const int*)p;
    RT_HIP(last_hip, hipMemcpyAsync(p, xy, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  } else {
    q.origins = (const float*)p;
    q.dirs = (const float*)(p + v3);
    RT_HIP(last_hip, hipMemcpyAsync(p, origins, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    RT_HIP(last_hip, hipMemcpyAsync(p + v3, dirs, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  }
  p += in_bytes;
  if (t) q.t = (float*)p, p += v1;
  if (ind) q.ind = (int*)p, p += v1;
  if (normals) q.nrm = (float*)p, p += v3;
  if (xy && dir_out) q.dir_out = (float*)p, p += v3;
  RT_HIP(last_hip, launch_ray_query(q, st, tree, log));
  if (t) RT_HIP(last_hip, hipMemcpyAsync(t, q.t, n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (ind) RT_HIP(last_hip, hipMemcpyAsync(ind, q.ind, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (normals) RT_HIP(last_hip, hipMemcpyAsync(normals, q.nrm, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (q.dir_out) RT_HIP(last_hip, hipMemcpyAsync(dir_out, q.dir_out, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  RT_HIP(last_hip, hipStreamSynchronize(st));
  return RT_OK;
}

int QueryWork::occluded(const QueryScene& sc, const QueryTree* tree, const float* from, const float* to, size_t n, uint8_t* out,
                        hipStream_t st, int& last_hip) {
  const size_t v3 = part(n * 3 * sizeof(float));
  int rc = reserve(2 * v3 + part(n), last_hip);
  if (rc != RT_OK) return rc;
  unsigned char* p = d_buf;
  RT_HIP(last_hip, hipMemcpyAsync(p, from, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  RT_HIP(last_hip, hipMemcpyAsync(p + v3, to, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  RT_HIP(last_hip, launch_occluded(sc, (const float*)p, (const float*)(p + v3), n, p + 2 * v3, st, tree, log));
  RT_HIP(last_hip, hipMemcpyAsync(out, p + 2 * v3, n, hipMemcpyDeviceToHost, st));
  RT_HIP(last_hip, hipStreamSynchronize(st));
  return RT_OK;
}

}  // namespace rt
