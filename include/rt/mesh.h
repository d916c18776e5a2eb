/* include/rt/mesh.h — triangle meshes: ray queries over a box hierarchy, and OBJ input.
 *
 * A companion to include/rt/abi.h, exported by librtrt_mesh.so (not by librtrt.so): a mesh is
 * uploaded once, a box hierarchy (BVH) over its triangles is built on the host, and closest-hit and
 * occlusion queries run on the GPU, one ray per lane.  The queries can be merged with the scene's own
 * answers (rt_trace_rays / rt_trace_pixels / rt_occluded and their _device forms) on one stream, e.g.
 * rt_get_stream(ctx).  Nothing here renders; the frame programs do not see meshes.
 *
 * Conventions are abi.h's: every function returns an RT_* status unless it says otherwise; an
 * rt_mesh is not thread-safe; the _host functions and rt_obj_parse never touch the GPU.
 *
 * ---- The rule ----------------------------------------------------------------------------------
 * Stated here once, specified in C by the _host functions (csrc/rt_mesh_host.cpp), reproduced bit
 * for bit by the kernels (csrc/rt_mesh_kernels.hip).  Float semantics are the project's: binary32,
 * no contraction, dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), '/' and sqrt correctly
 * rounded; min(a, b) is (a < b ? a : b) and max(a, b) is (a > b ? a : b).
 *
 * A mesh is verts[nv][3] float32 and tris[nt][3] int32, nt <= RT_MESH_MAX_TRIANGLES.  An index
 * outside [0, nv) is RT_E_INVAL at creation.  A triangle with a non-finite vertex component is
 * dead: no ray ever hits it and it is left out of the hierarchy.
 *
 * Ray gate.  A ray with a non-finite component in its origin o or direction d hits nothing
 * (t = -1, not occluded).  d is used as given, not normalised.
 *
 * box_pass(o, d, lo, hi), used for a triangle's own box and for every node.  Per axis a:
 *   |d_a| < FLT_MIN (zero or subnormal): the axis passes iff lo_a <= o_a <= hi_a and contributes
 *     no interval;
 *   otherwise inv = 1.0f / d_a, t1 = (lo_a - o_a) * inv, t2 = (hi_a - o_a) * inv (one subtraction,
 *     one multiplication each), near_a = min(t1, t2), far_a = max(t1, t2).
 * tn = max near_a and tf = min far_a over the contributing axes (x, y, z in turn; -inf and +inf
 * with none).  The box passes iff every zero axis passes, tf >= 0 and
 * tn <= tf * 1.000003814697265625f (1 + 2^-18).  Finite inputs produce no NaN here.
 *
 * tri_eval(o, d, v0, v1, v2) -> (t, u, v), t = -1 for a miss:
 *   1. the box gate: lo / hi = the componentwise min / max of v0, v1, v2 (exact); a miss if
 *      !box_pass(o, d, lo, hi);
 *   2. Moeller-Trumbore, cross(a, b).x = a.y * b.z - a.z * b.y (two products, one subtraction;
 *      cyclically for y and z):
 *        e1 = v1 - v0, e2 = v2 - v0, p = cross(d, e2), det = dot(e1, p); a miss if !(det != 0);
 *        inv = 1.0f / det, s = o - v0, u = dot(s, p) * inv; a miss if !(u >= 0 && u <= 1);
 *        q = cross(s, e1), v = dot(d, q) * inv; a miss if !(v >= 0 && u + v <= 1);
 *        t = dot(e2, q) * inv.
 * Both faces are hit.  A NaN anywhere fails a comparison: a miss.  The rule is NOT watertight along
 * shared edges: a ray aimed exactly at an edge may miss both of its triangles.
 *
 * Closest hit: over the live triangles i ascending, accept t_i > thr && (t_i < best || best < 0):
 * the lowest index wins a tie.  The hierarchy visits in another order and merges by (t, index),
 * which gives the same answer.  thr must be finite and >= 0.  Per ray: t; prim, the triangle's
 * index (-1: a miss); normal = normalize(cross(e1, e2)), the stored orientation, never flipped
 * (zeros for a miss); uv = (u, v) (zeros for a miss).
 *
 * Occlusion of the segment a -> b is rt_occluded's rule with tri_eval as eval_ray:
 * l = normalize(b - a), len = length(b - a), o = a + 0.01f * l (the ray gate applies to o and l);
 * occluded iff some live triangle has t, widened to binary64, with t > 0.0001f and
 * length(dvec3(t * l)) < len.
 *
 * Why the gate is part of the rule: a node's box is the exact componentwise min / max of the boxes
 * below it, and box_pass is monotone under containment (rounding is monotone; a zero axis is an
 * interval test): a ray that fails a box fails every box inside it.  So a node the walk skips holds
 * no triangle the brute-force loop accepts, and "walk = brute force, bit for bit" needs no error
 * analysis of Moeller-Trumbore.
 *
 * ---- The hierarchy -----------------------------------------------------------------------------
 * Deterministic, host only.  The live triangles' centroid keys are c = (v0 + v1) + v2 per component
 * (not divided).  A range of fewer than RT_MESH_SINGLE_LEAF (8) live triangles at the root is one
 * leaf node.  Otherwise a range of at most RT_MESH_LEAF (4) is a leaf (members in ascending index),
 * and a longer one is sorted by (key along the widest axis of the range's key bounds, index) and cut
 * at its median, the lower half first.  Nodes lie in preorder with skip links: a walk at node k
 * goes to k + 1 when the box passes (after testing the members if k is a leaf), else to skip[k];
 * it needs no stack and ends at k == nodes.  Nothing is pruned by the closest t found so far.
 */
#ifndef RT_MESH_H
#define RT_MESH_H

#include "abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MESH_MAX_TRIANGLES (1 << 24)
#define RT_MESH_LEAF 4        /* most members of a leaf below an inner node */
#define RT_MESH_SINGLE_LEAF 8 /* fewer live triangles than this: one leaf node holds them all */

/* query flags */
#define RT_MESH_ONE_ORIGIN 1 /* origins is one [3], used for every ray */
#define RT_MESH_MERGE 2      /* the outputs hold an earlier answer; see rt_mesh_trace_rays */

typedef struct rt_mesh rt_mesh;

/* ---- lifetime ---------------------------------------------------------------------------------- */
/* Checks the indices, builds the hierarchy on the host, allocates the device buffers on `device`
 * and uploads them, once; creates the mesh's own stream.  nt = 0 (verts and tris may then be NULL)
 * and a mesh without a live triangle are valid: every query misses.  RT_E_INVAL: a NULL out, nv < 0,
 * nt < 0 or above RT_MESH_MAX_TRIANGLES, a NULL array that is needed, an index outside [0, nv).
 * RT_E_NODEV: no such device. */
int rt_mesh_create(int device, const float* verts, int nv, const int32_t* tris, int nt, rt_mesh** out);
int rt_mesh_destroy(rt_mesh* mesh); /* waits for the mesh's own stream; NULL is RT_E_INVAL */

/* nodes and leaves of the hierarchy, dead triangles, bytes of the mesh's device buffers (without the
 * workspace).  Any output may be NULL. */
int rt_mesh_stats(const rt_mesh* mesh, int* nodes, int* leaves, int* dead, size_t* bytes);
/* the hipError_t of the last failed HIP call of this mesh (0: none) */
int rt_mesh_last_hip_error(const rt_mesh* mesh);
/* bytes of the host-pointer queries' device workspace: 0 until the first such query, grown only when
 * a call needs more, untouched by the _device queries.  0 for NULL. */
size_t rt_mesh_workspace_bytes(const rt_mesh* mesh);

/* ---- queries on the GPU ---------------------------------------------------------------------- */
/* Closest hits of n rays, host pointers: origins [n][3] ([3] with RT_MESH_ONE_ORIGIN), dirs [n][3];
 * outputs t [n], prim [n], normals [n][3], uv [n][2], any of them NULL when not wanted.  Staged
 * through the mesh's workspace on the mesh's own stream; waits before returning.
 * RT_MESH_MERGE: t (required) and normals are in-out and hold an earlier answer, e.g. the scene's.
 * The mesh's hit replaces it only where the existing t < 0 or the mesh's t is strictly less (the
 * earlier answer wins ties, and stands where its t is NaN); where it stands, prim is -1, uv zeros,
 * and t and normals keep their values.
 * n = 0 is RT_OK.  RT_E_INVAL: a NULL mesh, a NULL input with n > 0, n > RT_QUERY_MAX_RAYS, thr not
 * finite or < 0, an unknown flag bit, RT_MESH_MERGE with a NULL t. */
int rt_mesh_trace_rays(rt_mesh* mesh, const float* origins, const float* dirs, size_t n, int flags, float thr,
                       float* t, int32_t* prim, float* normals, float* uv);
/* Occlusion of the n segments from[i] -> to[i] ([n][3] each): out[i] = 1 if occluded, else 0.
 * RT_MESH_MERGE: out is in-out, the mesh's answer is OR-ed into it (any non-zero byte becomes 1).
 * RT_MESH_ONE_ORIGIN is not a flag of this query.  A NULL out with n > 0 does nothing (RT_OK), with
 * RT_MESH_MERGE it is RT_E_INVAL. */
int rt_mesh_occluded(rt_mesh* mesh, const float* from, const float* to, size_t n, int flags, uint8_t* out);

/* The same on device pointers, enqueued on hip_stream (a hipStream_t of the mesh's device, e.g.
 * rt_get_stream(ctx); NULL: the mesh's own stream): no allocation, no host wait, no event or stream
 * is created.  The buffers must stay valid until the stream reaches the work. */
int rt_mesh_trace_rays_device(rt_mesh* mesh, void* hip_stream, const float* d_origins, const float* d_dirs, size_t n,
                              int flags, float thr, float* d_t, int32_t* d_prim, float* d_normals, float* d_uv);
int rt_mesh_occluded_device(rt_mesh* mesh, void* hip_stream, const float* d_from, const float* d_to, size_t n,
                            int flags, uint8_t* d_out);
/* waits for the mesh's own stream */
int rt_mesh_synchronize(rt_mesh* mesh);

/* ---- the specification, host only ---------------------------------------------------------------- */
/* tri_eval: returns t (-1: a miss, also for a NULL argument); uv (may be NULL) gets (u, v), zeros for
 * a miss.  Evaluates the rule as written, whatever the vertices hold. */
float rt_mesh_tri_eval_host(const float o[3], const float d[3], const float v0[3], const float v1[3],
                            const float v2[3], float uv[2]);
/* box_pass: 1 or 0 (0 for a NULL argument) */
int rt_mesh_box_pass_host(const float o[3], const float d[3], const float lo[3], const float hi[3]);
/* rt_mesh_trace_rays / rt_mesh_occluded by brute force: every live triangle in index order, no
 * hierarchy; same flags, same argument checks (plus those of rt_mesh_create on the mesh). */
int rt_mesh_trace_rays_host(const float* verts, int nv, const int32_t* tris, int nt, const float* origins,
                            const float* dirs, size_t n, int flags, float thr, float* t, int32_t* prim,
                            float* normals, float* uv);
int rt_mesh_occluded_host(const float* verts, int nv, const int32_t* tris, int nt, const float* from,
                          const float* to, size_t n, int flags, uint8_t* out);
/* The hierarchy rt_mesh_create builds: boxes [nodes][6] (lo.xyz, hi.xyz), links [nodes][3] (skip,
 * first, count; count 0: an inner node, else the leaf's members are leaf_index[first, first + count)),
 * leaf_index [live]: the live triangles' indices in leaf order.  Returns the number of nodes (0: no
 * live triangle), *live the number of live triangles; -1 for a bad argument or a capacity too small
 * (node_cap < nodes or leaf_cap < live; 2 * nt nodes and nt entries always suffice). */
int rt_mesh_bvh_host(const float* verts, int nv, const int32_t* tris, int nt, float* boxes, int32_t* links,
                     int node_cap, int32_t* leaf_index, int leaf_cap, int* live);

/* ---- OBJ input, host only -------------------------------------------------------------------- */
/* Reads the geometry of a Wavefront OBJ text of `bytes` bytes (no terminator needed): `v x y z [w]`
 * (w ignored) and `f` with vertices written i, i/j, i/j/k or i//k (only i is used; 1-based, negative:
 * relative to the vertices read so far); a polygon of m vertices becomes the fan (0, k, k + 1),
 * k = 1 .. m - 2.  Comments (#), blank lines, CRLF line ends and every other statement (vn, vt, g, o,
 * s, usemtl, mtllib ...) are skipped.  *nv and *nt get the counts; vertices and triangles are stored
 * while they fit in vcap / tcap (verts and tris may be NULL with a zero cap): call once with zero caps
 * to size the arrays and again to fill them.  Triangle indices are 0-based.
 * RT_E_INVAL with *err_line (1-based; 0: a bad argument) for a malformed line: a number that does not
 * parse, a v with fewer than three numbers, an f with fewer than three vertices, index 0, an index
 * outside the vertices read so far, more than RT_MESH_MAX_TRIANGLES triangles. */
int rt_obj_parse(const char* text, size_t bytes, float* verts, int vcap, int32_t* tris, int tcap, int* nv,
                 int* nt, int* err_line);

#ifdef __cplusplus
}
#endif
#endif /* RT_MESH_H */
