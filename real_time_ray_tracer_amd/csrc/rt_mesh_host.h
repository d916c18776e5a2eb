// rt_mesh_host.h — what rt_mesh.hip takes from the host-only unit rt_mesh_host.cpp: the checked
// mesh, its hierarchy and the tables as the kernels read them.  No HIP header.
#pragma once
#include <cstdint>
#include <vector>

namespace rt {
namespace mesh {

struct Bvh {
  std::vector<float> boxes;    // [nodes][6]: lo.xyz, hi.xyz
  std::vector<int32_t> links;  // [nodes][3]: skip, first, count (0: an inner node)
  std::vector<int32_t> order;  // [live]: the live triangles in leaf order
  int nodes = 0, leaves = 0, dead = 0;
};

// RT_OK, or RT_E_INVAL for what rt_mesh_create refuses
int check_mesh(const float* verts, int nv, const int32_t* tris, int nt);
// the deterministic build (include/rt/mesh.h "The hierarchy") of a checked mesh
void build_bvh(const float* verts, const int32_t* tris, int nt, Bvh& out);
// what the walk relies on: skip links strictly increasing and at most `nodes`, leaf ranges inside the
// table, counts within the packing's 4 bits
bool bvh_valid(const Bvh& b);
// the device tables: nodes [nodes][8] floats (lo.xyz, bits of skip, hi.xyz, bits of first * 16 + count),
// tris [live][12] floats in leaf order (v0.xyz, bits of the index, v1.xyz, 0, v2.xyz, 0)
void pack_tables(const float* verts, const int32_t* tris, const Bvh& b, std::vector<float>& nodes,
                 std::vector<float>& leaf_tris);

}  // namespace mesh
}  // namespace rt
