// rt_timing.hip — launch timing (rt_timing.h).
#include "rt_timing.h"

namespace rt {
namespace {

hipEvent_t get_event(std::vector<hipEvent_t>& pool) {
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

}  // namespace

int LaunchTiming::begin(Timed& t, hipStream_t st, int& last_hip) {
  t.e0 = get_event(event_pool);
  t.e1 = get_event(event_pool);
  if (!t.e0 || !t.e1) return RT_E_HIP;
  RT_HIP(last_hip, hipEventRecord(t.e0, st));
  return RT_OK;
}

int LaunchTiming::end(int program, const Timed& t, hipStream_t st, int& last_hip) {
  RT_HIP(last_hip, hipEventRecord(t.e1, st));
  pending[program].push_back(t);
  return RT_OK;
}

bool LaunchTiming::any_pending() const {
  for (auto& p : pending)
    if (!p.empty()) return true;
  return false;
}

int LaunchTiming::resolve(int& last_hip) {
  for (int k = 0; k < RT_PROG_COUNT; ++k) {
    for (auto& pr : pending[k]) {
      float ms = 0.0f;
      RT_HIP(last_hip, hipEventElapsedTime(&ms, pr.e0, pr.e1));
      total_ms[k] += ms;
      launches[k] += pr.frames;  // per frame: a multi-frame launch counts its frames
      event_pool.push_back(pr.e0);
      event_pool.push_back(pr.e1);
    }
    pending[k].clear();
  }
  return RT_OK;
}

void LaunchTiming::reset() {
  for (int k = 0; k < RT_PROG_COUNT; ++k) {
    total_ms[k] = 0.0;
    launches[k] = 0;
  }
}

void LaunchTiming::release() {
  for (auto& p : pending)
    for (auto& pr : p) {
      (void)hipEventDestroy(pr.e0);
      (void)hipEventDestroy(pr.e1);
    }
  for (auto e : event_pool) (void)hipEventDestroy(e);
  *this = LaunchTiming{};
}

}  // namespace rt
