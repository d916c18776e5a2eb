// rt_timing.h — launch timing: an event pair around each launch while timing is on, resolved
// into per-program totals once the streams have been drained.
#pragma once
#include <vector>

#include "rt_hip_util.h"

namespace rt {

struct LaunchTiming {
  struct Timed {
    hipEvent_t e0, e1;
    int frames;  // frames the launch rendered (multi-frame Phong/hybrid launches: up to kMaxBatch)
  };
  bool on = false;                            // rt_enable_timing
  std::vector<Timed> pending[RT_PROG_COUNT];  // recorded on the launch stream
  std::vector<hipEvent_t> event_pool;
  double total_ms[RT_PROG_COUNT] = {};
  int launches[RT_PROG_COUNT] = {};

  // around a launch of `program` on st, while `on`: begin records the first event of the pair
  int begin(Timed& t, hipStream_t st, int& last_hip);
  int end(int program, const Timed& t, hipStream_t st, int& last_hip);
  bool any_pending() const;
  // the pending pairs into the totals; the caller has drained every stream they were recorded on
  int resolve(int& last_hip);
  void reset();  // the totals
  void release();
};

}  // namespace rt
