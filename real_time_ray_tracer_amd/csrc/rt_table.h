// rt_table.h — layout of the device shape table and the constants its packing needs, shared by
// the kernels (rt_kernels.h) and the host-only planning unit (rt_plan.cpp, no HIP header).
#pragma once
#include <stddef.h>

#if defined(__host__) && defined(__device__)  // after <hip/hip_runtime.h>; empty outside hipcc
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rt {

constexpr int kMaxBatch = 32;  // frames per multi-frame Phong/hybrid launch

// AO pools: kAoPool samples each, i.e. max(1, kAoPool / spp) consecutive pixels of the launch's rows
constexpr int kAoPool = 256;
constexpr long long ao_pool_count(int trace_rows, int W, int spp) {
  const int TP = kAoPool / spp > 0 ? kAoPool / spp : 1;
  return ((long long)trace_rows * W + TP - 1) / TP;
}

// Bounce-ray cluster culling (AO later bounce rounds): at most kMaxClusters clusters (a wave-uniform
// u64 of kept clusters), member masks over the first kClusterWords * 64 spheres.
constexpr int kMaxClusters = 64;
constexpr int kClusterWords = 4;

// Device shape table of one header copy, in float4 units from its base (rt_plan pack_header fills it):
//   [0, 4S)          geo, geo2, col, aux        (rt_device.h "scene tables")
//   [4S, 5S)         sph: geo of spheres, NaN of other shapes (never accepted by sphere_candidate)
//   [5S, 7S)         planes: 2 float4 per plane, compacted, ascending index
//   [7S, 7S + 64)    clusters: (centre, R) per cluster
//   then (1 + 64) * 4 u64 cluster masks (the always-tested spheres, then each cluster's members)
//   then [S) camrel: per sphere (camera - centre, dot of it with itself), NaN for other shapes:
//        the camera rays' sphere tests without the per-lane subtraction and self dot (phong /
//        hybrid primary rays; the same float operations, done once per frame on the host)
//   then rand_buffer[2 spp]
RT_HD constexpr size_t sphere_table(int S) { return (size_t)4 * S; }
RT_HD constexpr size_t plane_table(int S) { return (size_t)5 * S; }
RT_HD constexpr size_t cluster_table(int S) { return (size_t)7 * S; }
RT_HD constexpr size_t cluster_mask_table(int S) { return cluster_table(S) + kMaxClusters; }
RT_HD constexpr size_t camrel_table(int S) {
  return cluster_mask_table(S) + (size_t)(1 + kMaxClusters) * kClusterWords / 2;
}
RT_HD constexpr size_t rand_table(int S) { return camrel_table(S) + (size_t)S; }
RT_HD constexpr size_t table_vec4(int S, int spp) { return rand_table(S) + (size_t)2 * spp; }
// Rectangles in effect (rt_set_rectangles, include/rt/abi.h "Rectangles") enter the plane table in
// ascending index order with the planes, as (n, bits(index)), (llc, bits(offset)): offset != 0 is the
// distance in float4 from the plane table's base to the rectangle's two rows in a region appended to
// the table, [2 S) rows behind rand_buffer: (right, dot(right, right)), (up, dot(up, up)).  A plane's
// second row keeps w = 0.  Nothing above moves; a table packed without rectangles ends at table_vec4.
RT_HD constexpr size_t rect_table(int S, int spp) { return table_vec4(S, spp); }
RT_HD constexpr size_t table_vec4_rect(int S, int spp) { return rect_table(S, spp) + (size_t)2 * S; }

}  // namespace rt
