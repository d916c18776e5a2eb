// rt_cull.hip — the cull cache (rt_cull.h).
#include "rt_cull.h"

#include "rt_plan.h"

namespace rt {

int CullCache::invalidate(int& last_hip) {
  list_pending = list_ready = false;  // (a copy of counts still in flight is the old fill's: ev_list is recorded anew)
  if (!valid) return RT_OK;
  valid = false;
  for (auto& s : readers.s) {
    if (!s) continue;
    if (!ev_read[n_read]) RT_HIP(last_hip, hipEventCreateWithFlags(&ev_read[n_read], hipEventDisableTiming));
    RT_HIP(last_hip, hipEventRecord(ev_read[n_read], s));
    ++n_read;
    s = nullptr;
  }
  return RT_OK;
}

void CullCache::streams_idle() {
  n_read = 0;
  readers.clear();
  seen.clear();
}

void CullCache::release() {
  if (d_alloc) (void)hipFree(d_alloc);
  if (ev_fill) (void)hipEventDestroy(ev_fill);
  if (ev_list) (void)hipEventDestroy(ev_list);
  if (h_counts) (void)hipHostFree(h_counts);
  for (auto e : ev_read)
    if (e) (void)hipEventDestroy(e);
  *this = CullCache{};
}

int CullCache::before(const rt_config& cfg, const float* h, FrameParams& p, hipStream_t st, int& last_hip) {
  p.cull = nullptr;
  p.cull_frames = 0;
  const int nwmax = (cfg.num_shapes + 63) / 64;
  const size_t need = (size_t)ao_pool_count(p.trace_rows, p.W, p.spp) * nwmax * sizeof(unsigned long long);
  const bool whole_band = p.trace_row0 == p.band_row0 && p.trace_rows == p.band_rows;  // (every AO launch's rows)
  if (!on || nomem || p.nplanes > 0 || p.nobj <= 0 || !whole_band || need == 0 || need > cap) {
    have_key = false;
    return invalidate(last_hip);
  }
  next.resize(cull_key(cfg, h, nullptr, 0));
  if (next.empty() || cull_key(cfg, h, next.data(), next.size()) != next.size()) {
    have_key = false;
    return invalidate(last_hip);
  }
  if (!have_key || next != key) {
    key.swap(next);
    have_key = true;
    repeats = 0;
    return invalidate(last_hip);
  }
  if (++repeats < kCullRepeats) return RT_OK;
  repeats = kCullRepeats;
  const bool filled_now = !valid;
  if (!valid) {
    if (!d_table) {  // lazily; a failed allocation leaves the context uncached
      // masks and sort frames in one allocation when both fit the cap, else (or when that
      // allocation fails) the masks alone
      // and the pool list in front of both when all three fit (and its pinned counts can be had)
      const long long pools = ao_pool_count(p.trace_rows, p.W, p.spp);
      size_t fb = ao_cull_frame_bytes(pools);
      if (fb > cap - need) fb = 0;
      size_t lb = fb != 0 ? ao_pool_list_bytes(pools) : 0;
      if (lb > cap - need - fb) lb = 0;
      if (lb != 0 && !h_counts && hipHostMalloc((void**)&h_counts, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        h_counts = nullptr;
        lb = 0;
      }
      hipError_t e = hipMalloc(&d_alloc, lb + fb + need);
      if (e != hipSuccess && lb != 0) {
        (void)hipGetLastError();
        lb = 0;
        e = hipMalloc(&d_alloc, fb + need);
      }
      if (e != hipSuccess && fb != 0) {
        (void)hipGetLastError();
        fb = 0;
        e = hipMalloc(&d_alloc, need);
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();
        d_alloc = nullptr;
        nomem = true;
        return RT_OK;
      }
      list_bytes = lb;
      list_pools = lb != 0 ? pools : 0;
      frame_bytes = fb;
      d_table = (unsigned long long*)((char*)d_alloc + lb + fb);
      bytes = need;
    }
    if (!ev_fill) RT_HIP(last_hip, hipEventCreateWithFlags(&ev_fill, hipEventDisableTiming));
    for (int s = 0; s < n_read; ++s) RT_HIP(last_hip, hipStreamWaitEvent(st, ev_read[s], 0));
    n_read = 0;
    RT_HIP(last_hip, launch_cull_fill(p, d_table, frame_bytes != 0, st, log));
    if (list_bytes != 0 && list_on) {  // the list, then its counts to the host; ev_fill covers both
      if (!ev_list) RT_HIP(last_hip, hipEventCreateWithFlags(&ev_list, hipEventDisableTiming));
      RT_HIP(last_hip, launch_pool_list(p, d_table, st));
      RT_HIP(last_hip, hipMemcpyAsync(h_counts, (char*)d_table - frame_bytes - 16, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
      RT_HIP(last_hip, hipEventRecord(ev_list, st));
      list_pending = true;
      list_builds += 1;
    }
    RT_HIP(last_hip, hipEventRecord(ev_fill, st));
    seen.clear();
    seen.s[0] = st;
    valid = true;
    fills += 1;
  }
  if (seen.add(st)) RT_HIP(last_hip, hipStreamWaitEvent(st, ev_fill, 0));
  readers.add(st);
  p.cull = d_table;
  p.cull_frames = frame_bytes != 0;
  cached += 1;
  if (list_pending && !filled_now) {  // polled, never waited for (the launch behind the build: over every pool)
    bool landed = false;
    RT_HIP(last_hip, event_done(hipEventQuery(ev_list), landed));
    if (landed) {
      list_pending = false;
      list_ready = true;
    }
  }
  if (list_ready && list_on && ao_takes_pool_list(p)) {
    p.cull_frames = 2;
    p.pool_rot = h_counts[0];
    list_launches += 1;
  }
  return RT_OK;
}

}  // namespace rt
