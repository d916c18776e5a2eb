// rt_sched.h — the longest-first workgroup schedule of the hybrid (mode 4) launches.
#pragma once
#include <vector>

#include "rt_hip_util.h"
#include "rt_kernels.h"

namespace rt {

// Longest-first workgroup schedule.  A launch's time is set by its longest workgroups when they
// start late: the few hybrid tiles (mode 4) whose mirror paths bounce for many rounds.  The waves
// record their bounce rounds in d_cost; every kSchedPeriod-th launch the costs are read back on
// a side stream, and when the sorted order changes it is uploaded into the table no launch in
// flight reads, which becomes the active one once the copy has landed.  Nothing here waits on the GPU or puts a copy between two launches
// on a launch stream; the permutation only moves work between workgroups, so the images do not
// depend on it.
// (AO pools in the same longest-first order by wave time measured nothing at (c) and (d): those
// launches are not tail-bound; the kernel's bookkeeping cost registers, profiles/r04h_*)
constexpr int kSchedPeriod = 16;
struct TileSched {
  bool on = true;                      // rt_set_tile_schedule
  int gx = 0, gy = 0, nunits = 0, per_unit = 1;  // units (tiles) = gx * gy; cost slots per unit; nunits != 0: set up
  unsigned* d_cost = nullptr;          // [nunits * per_unit]
  unsigned* d_order[2] = {};           // [nunits] each
  unsigned* h_cost = nullptr;          // pinned
  unsigned* h_order[2] = {};           // pinned
  hipStream_t side = nullptr;
  hipEvent_t ev_launch = nullptr, ev_cost = nullptr, ev_order = nullptr;
  hipEvent_t ev_use[2][kAoStreams] = {};  // per table: its last readers on each launch stream
  StreamSet used_on[2];                // the launch streams a table was read on
  int active = -1;                     // the table launches read (-1: the plain order)
  int pending = -1;                    // the table being uploaded
  bool cost_inflight = false;
  long long launches = 0;
  int orders_taken = 0;                // orders that became active (rt_tile_schedule_orders)
  std::vector<unsigned> cur, next;     // the active / pending order

  // Before a launch over gx x gy units (cost slots per_unit each) whose stream is ordered after
  // `main`: take up a landed order table, turn landed costs into an order (rt_plan sched_order),
  // and set the launch's tile_order / tile_cost.
  int before(int gx, int gy, int per_unit, hipStream_t main, FrameParams& p, int& last_hip);
  // After that launch on stream `st`: note that the active table was read on st; every
  // kSchedPeriod-th launch has its costs read back on the side stream (launches after it may
  // overwrite them meanwhile: a cost is a hint, never a result).
  int after(hipStream_t st, int& last_hip);
  // every launch stream has been drained: no launch reads an order table any more
  void forget_streams();
  // back to "not set up" (`on` is kept); the caller has made sure no launch in flight reads the tables
  void release();
};

}  // namespace rt
