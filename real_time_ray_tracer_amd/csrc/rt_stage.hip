// rt_stage.hip — the staging ring (rt_stage.h).
#include "rt_stage.h"

#include <chrono>
#include <cstring>

namespace rt {

int StageRing::copy(void* dst, const void* src, size_t bytes, hipStream_t st, int& last_hip) {
  if (bytes == 0) return RT_OK;
  Slot& s = slot[next];
  next = (next + 1) % kStageSlots;
  if (s.used) {
    // not done: the GPU has not consumed it yet (wait); a failed query is a fault of the copy or
    // of the work before it on the stream: reported, never taken as "consumed" and the buffer reused
    hipError_t q = hipEventQuery(s.done);
    if (inject_query_error) {
      q = (hipError_t)inject_query_error;
      inject_query_error = 0;
    }
    bool consumed = false;
    RT_HIP(last_hip, event_done(q, consumed));
    if (!consumed) {
      const auto t0 = std::chrono::steady_clock::now();
      RT_HIP(last_hip, hipEventSynchronize(s.done));
      wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      waits += 1;
    }
  }
  if (s.bytes < bytes) {  // grow to a power of two >= 256 KiB: pinned allocations are slow, keep them rare
    if (s.host) RT_HIP(last_hip, hipHostFree(s.host));
    s.host = nullptr;
    size_t cap = 256 << 10;
    while (cap < bytes) cap <<= 1;
    RT_HIP(last_hip, hipHostMalloc(&s.host, cap, hipHostMallocDefault));
    s.bytes = cap;
  }
  if (!s.done) RT_HIP(last_hip, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  std::memcpy(s.host, src, bytes);
  RT_HIP(last_hip, hipMemcpyAsync(dst, s.host, bytes, hipMemcpyHostToDevice, st));
  RT_HIP(last_hip, hipEventRecord(s.done, st));
  s.used = true;
  return RT_OK;
}

void StageRing::release() {
  for (auto& s : slot) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.host) (void)hipHostFree(s.host);
    s = Slot{};
  }
}

}  // namespace rt
