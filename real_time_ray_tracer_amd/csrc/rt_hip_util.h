// rt_hip_util.h — the idioms the shim and its components share: error recording, the event
// query, lazy allocation and the small stream set.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rt/abi.h"

namespace rt {

// AO streams: pipelined frame k's AO pass runs on AO stream k % n_ao_streams (0 = the main
// stream) and reads header copy k % n_ao_streams
constexpr int kAoStreams = 3;  // capacity; in use: the context's n_ao_streams (default 2)

// A failed HIP call: recorded where rt_last_hip_error finds it (`last`: the context's last_hip)
inline int hip_fail(int& last, hipError_t e) {
  last = (int)e;
  return RT_E_HIP;
}

#define RT_HIP(where, expr)                           \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return hip_fail(where, _e); \
  } while (0)

// Has the work before an event finished?  q is hipEventQuery's answer: hipErrorNotReady is "not
// yet" (its per-thread error is cleared); any other failure is a fault of the work the event
// follows, returned for the caller to report (rt_last_hip_error), never taken as "not yet" or "done"
inline hipError_t event_done(hipError_t q, bool& done) {
  done = q == hipSuccess;
  if (q == hipErrorNotReady) {
    (void)hipGetLastError();
    return hipSuccess;
  }
  return q;
}

// Allocate a buffer that is made lazily: out of memory becomes RT_E_NOMEM with the error recorded
// and the pointer nulled, any other failure RT_E_HIP
template <class T>
int alloc_or_nomem(T** p, size_t bytes, int& last) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {
    last = (int)e;
    *p = nullptr;
    return RT_E_NOMEM;
  }
  RT_HIP(last, e);
  return RT_OK;
}

// The few streams something was enqueued on since the last drain
struct StreamSet {
  hipStream_t s[kAoStreams] = {};
  bool add(hipStream_t st) {  // false if it was there
    for (auto& x : s) {
      if (x == st) return false;
      if (!x) {
        x = st;
        return true;
      }
    }
    s[0] = st;  // (never: a context launches on at most kAoStreams streams between two drains)
    return true;
  }
  void clear() {
    for (auto& x : s) x = nullptr;
  }
};

}  // namespace rt
