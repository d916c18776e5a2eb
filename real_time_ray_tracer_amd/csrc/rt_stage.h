// rt_stage.h — the staging ring: async host-to-device copies through pinned buffers.
#pragma once
#include "rt_hip_util.h"

namespace rt {

constexpr int kStageSlots = 8;

struct StageRing {
  struct Slot {
    void* host = nullptr;  // pinned
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
  };
  Slot slot[kStageSlots];
  int next = 0;
  int inject_query_error = 0;  // test hook (rt_debug_fail_next_event_query): the next query fails
  // host time spent waiting for a staging buffer to be free (back-pressure: the host is up to
  // kStageSlots uploads ahead of the GPU), since the last reset_stats
  double wait_ms = 0.0;
  long long waits = 0;

  // Async H2D copy through the ring, so callers may reuse their (pageable) memory as soon as the
  // call returns and the stream never has to drain.
  int copy(void* dst, const void* src, size_t bytes, hipStream_t st, int& last_hip);
  void reset_stats() { wait_ms = 0.0, waits = 0; }
  void release();
};

}  // namespace rt
