// rt_sched.hip — the longest-first tile schedule (rt_sched.h).
#include "rt_sched.h"

#include <cstring>

#include "rt_plan.h"

namespace rt {
namespace {

hipError_t setup(TileSched& h, int gx, int gy, int per_unit, hipStream_t main) {
  const int nunits = gx * gy;
  const size_t nc = (size_t)nunits * per_unit * sizeof(unsigned), no = (size_t)nunits * sizeof(unsigned);
  hipError_t e = hipMalloc(&h.d_cost, nc);
  if (e == hipSuccess) e = hipMemsetAsync(h.d_cost, 0, nc, main);
  if (e == hipSuccess) e = hipHostMalloc(&h.h_cost, nc, hipHostMallocDefault);
  for (int k = 0; k < 2; ++k) {
    if (e == hipSuccess) e = hipMalloc(&h.d_order[k], no);
    if (e == hipSuccess) e = hipHostMalloc(&h.h_order[k], no, hipHostMallocDefault);
    for (auto& ev : h.ev_use[k])
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h.side, hipStreamNonBlocking);
  for (hipEvent_t* ev : {&h.ev_launch, &h.ev_cost, &h.ev_order})
    if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  h.gx = gx;
  h.gy = gy;
  h.per_unit = per_unit;
  h.nunits = nunits;  // set up, all of it
  return hipSuccess;
}

}  // namespace

void TileSched::release() {
  if (side) (void)hipStreamSynchronize(side);
  if (d_cost) (void)hipFree(d_cost);
  for (int k = 0; k < 2; ++k) {
    if (d_order[k]) (void)hipFree(d_order[k]);
    if (h_order[k]) (void)hipHostFree(h_order[k]);
    for (auto e : ev_use[k])
      if (e) (void)hipEventDestroy(e);
  }
  if (h_cost) (void)hipHostFree(h_cost);
  for (auto e : {ev_launch, ev_cost, ev_order})
    if (e) (void)hipEventDestroy(e);
  if (side) (void)hipStreamDestroy(side);
  const bool keep = on;
  *this = TileSched{};
  on = keep;
}

void TileSched::forget_streams() {
  for (auto& u : used_on) u.clear();
}

int TileSched::before(int ngx, int ngy, int nper, hipStream_t main, FrameParams& p, int& last_hip) {
  if (!on || ngx < 1 || ngy < 1) return RT_OK;
  if (nunits && (gx != ngx || gy != ngy || per_unit != nper)) {
    RT_HIP(last_hip, hipDeviceSynchronize());  // (never in practice: a context's launch shapes are fixed)
    release();
  }
  if (!nunits) {
    if (ngx >= 65536 || ngy >= 65536) return RT_OK;
    const hipError_t e = setup(*this, ngx, ngy, nper, main);
    if (e != hipSuccess) {  // all or nothing: the next launch finds it not set up, and tries again
      release();
      return hip_fail(last_hip, e);
    }
  }
  bool order_landed = false, cost_landed = false;
  if (pending >= 0) RT_HIP(last_hip, event_done(hipEventQuery(ev_order), order_landed));
  if (cost_inflight) RT_HIP(last_hip, event_done(hipEventQuery(ev_cost), cost_landed));
  if (order_landed) {
    if (active >= 0)  // the launches enqueued so far are the old table's last readers
      for (int s = 0; s < kAoStreams; ++s)
        if (used_on[active].s[s]) RT_HIP(last_hip, hipEventRecord(ev_use[active][s], used_on[active].s[s]));
    active = pending;
    pending = -1;
    ++orders_taken;
    cur.swap(next);
    used_on[active].clear();
  }
  if (cost_landed) {
    cost_inflight = false;
    if (pending < 0 && sched_order(gx, gy, per_unit, h_cost, cur, next)) {
      const int x = active == 0 ? 1 : 0;  // the table no launch reads from now on
      const size_t bytes = next.size() * sizeof(unsigned);
      std::memcpy(h_order[x], next.data(), bytes);
      for (int s = 0; s < kAoStreams; ++s)
        if (used_on[x].s[s]) RT_HIP(last_hip, hipStreamWaitEvent(side, ev_use[x][s], 0));
      RT_HIP(last_hip, hipMemcpyAsync(d_order[x], h_order[x], bytes, hipMemcpyHostToDevice, side));
      RT_HIP(last_hip, hipEventRecord(ev_order, side));
      pending = x;
    }
  }
  p.tile_order = active >= 0 ? d_order[active] : nullptr;
  p.tile_cost = d_cost;
  return RT_OK;
}

int TileSched::after(hipStream_t st, int& last_hip) {
  if (!on || !nunits) return RT_OK;
  if (active >= 0) used_on[active].add(st);
  if (launches++ % kSchedPeriod == 0 && !cost_inflight) {
    RT_HIP(last_hip, hipEventRecord(ev_launch, st));
    RT_HIP(last_hip, hipStreamWaitEvent(side, ev_launch, 0));
    RT_HIP(last_hip, hipMemcpyAsync(h_cost, d_cost, (size_t)nunits * per_unit * sizeof(unsigned),
                                    hipMemcpyDeviceToHost, side));
    RT_HIP(last_hip, hipEventRecord(ev_cost, side));
    cost_inflight = true;
  }
  return RT_OK;
}

}  // namespace rt
