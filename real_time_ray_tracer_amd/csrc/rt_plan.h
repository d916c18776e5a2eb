// rt_plan.h — the shim's pure planning code: header validation and packing, the cull cache's key,
// the tile schedule's ordering step and rt_compute_frames' table-slot assignment.  No HIP: built by
// the plain compiler like rt_host.cpp (with -ffp-contract=off), so it also builds next to a
// stand-alone program under the host sanitizers (tests/test_plan_cpu.py).
#pragma once
#include <stddef.h>

#include <vector>

#include "../../include/rt/abi.h"
#include "rt_table.h"

namespace rt {

// One row of the device table: the bytes of a float4 (rt_shim.hip asserts it).
struct alignas(16) Row {
  float x, y, z, w;
};

// stride of the device shape tables (>= 1, so an empty scene still has valid pointers)
// One row per table beyond the shapes: the colour table's row -1 (the geo2 table's last row)
// holds the background, so the AO kernel's shading reads a miss's attenuation as col[-1]
// (rt_kernels_impl.h col_at) instead of keeping the background in scalar registers.
constexpr int table_stride(const rt_config& cfg) { return (cfg.num_shapes > 1 ? cfg.num_shapes : 1) + 1; }

// int(mode.z) of header h, the scene's object count: it must be in [0, S]; -1 when it is not
int header_nobj(const float* h, int S);

// Validate a header and pack it into the device table layout (rt::table_vec4 rows at `tab`:
// shape tables, sphere table, plane table, clusters, rand_buffer); sets nobj / nplanes / ncl.
int pack_header(const rt_config& cfg, const float* h, Row* tab, int& nobj, int& nplanes, int& ncl);
// The same with flags (RT_SCENE_RECTANGLES): the rectangles among [0, nobj) enter the plane table
// with the planes, ascending index, and their rows go to the appended region (rt_table.h
// rect_table); `tab` then holds rt::table_vec4_rect rows, the region's unused rows zero.  nplanes
// counts planes and rectangles, nrects the rectangles.  flags = 0 is the form above: nothing beyond
// rt::table_vec4 is read or written.
int pack_header(const rt_config& cfg, const float* h, Row* tab, int& nobj, int& nplanes, int& ncl, int flags,
                int& nrects);

// Bounce-ray clusters of the sphere table `sph` (see rt_plan.cpp); returns the cluster count.
int build_clusters(const Row* sph, int nobj, Row* ctab, unsigned long long* cmask);

// The ray queries' bounding-ball tree over the spheres (include/rt/abi.h "Query tree"; rt_plan.cpp).
// Leaves hold at most kTreeLeaf spheres: 4, the linear scan's rows per load (2 and 8 measured at 2048
// spheres, DESIGN.md §5 "Round 18").
#ifndef RT_TREE_LEAF
#define RT_TREE_LEAF 4  // (A/B builds override it)
#endif
constexpr int kTreeLeaf = RT_TREE_LEAF;
static_assert(kTreeLeaf >= 1, "a leaf holds at least one sphere");
// Most nodes of a tree over n members: every leaf holds at least one, so at most n leaves.
constexpr int tree_max_nodes(int n) { return n > 0 ? 2 * n - 1 : 0; }
struct TreeLink {
  int skip, first, count, pad;  // next node not below this one; a leaf's entries [first, first + count); an inner node: count 0
};
struct QueryTreeHost {
  std::vector<Row> ball;       // [nodes] (centre, R), preorder
  std::vector<TreeLink> link;  // [nodes]
  std::vector<Row> rows;       // the leaf table: sphere rows in leaf order, then the always list's rows
  std::vector<int> index;      // the entries' sphere indices
  int n_leaf_entries = 0, n_always = 0, n_leaves = 0;
  void reserve(int num_shapes);  // room for every tree over num_shapes rows: no build allocates afterwards
};
// Builds the tree of the sphere table `sph` over [0, nobj) into t; returns the node count, 0 = no tree
// (fewer than 2 * kTreeLeaf members; t is then empty).
int build_query_tree(const Row* sph, int nobj, QueryTreeHost& t);

// The cull cache's key of a context configuration (rows resolved: row_begin < row_end) and header
// h: the exact bytes of every input of the AO pool start's primary-ray cull (rt_cull.h) and the
// launch's pool count.  Written to `out` when it fits in cap bytes; returns the key's size, 0 for a
// header whose int(mode.z) is out of range.
size_t cull_key(const rt_config& cfg, const float* h, unsigned char* out, size_t cap);

// The tile schedule's ordering step: the gx x gy units longest first, a unit's cost being its
// slowest slot's among cost[unit * per_unit ..]; ties keep the plain order; packed x | y << 16 into
// `next`.  False ("none") when the costs are uniform or the order equals `cur`.
bool sched_order(int gx, int gy, int per_unit, const unsigned* cost, const std::vector<unsigned>& cur,
                 std::vector<unsigned>& next);

// rt_compute_frames' table slots of a batch of m frames.  same[j]: frame j's packed table equals
// the previous frame's (frame 0: the context's current table, which sits in slot `prev`; ignored
// when prev is -1).  Equal neighbours share a slot; the new tables take consecutive slots from the
// returned base, never over `prev` when frame 0 reads it (nslots >= 2 m).
int batch_slots(const unsigned char* same, int m, int prev, int nslots, int* slot);

}  // namespace rt
