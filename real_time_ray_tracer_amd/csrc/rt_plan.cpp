// rt_plan.cpp — the shim's pure planning code (rt_plan.h).  No HIP header; built with
// -ffp-contract=off: pack_header's camera-relative rows are the kernels' binary32 operations.
#include "rt_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>

namespace rt {

int header_nobj(const float* h, int S) {
  const float mz = h[RT_HDR_MODE * 4 + 2];
  return mz >= 0.0f && mz < (float)(S + 1) ? (int)mz : -1;
}

size_t cull_key(const rt_config& cfg, const float* h, unsigned char* out, size_t cap) {
  const int nobj = header_nobj(h, cfg.num_shapes);
  if (nobj < 0) return 0;
  const int band0 = std::max(0, cfg.row_begin - 1);
  const int band_rows = std::min(cfg.height, cfg.row_end + 1) - band0;  // the AO launches' rows (strip + halo)
  const long long pools = ao_pool_count(band_rows, cfg.width, cfg.spp);
  // (pool_rot is a function of W and spp, rt_kernels_impl.h launch_params)
  const int ints[6] = {cfg.width, cfg.height, band0, band_rows, cfg.spp, nobj};
  const float dims[2] = {(float)cfg.width, (float)cfg.height};
  size_t n = 0;
  auto put = [&](const void* src, size_t bytes) {
    if (out && n + bytes <= cap) std::memcpy(out + n, src, bytes);
    n += bytes;
  };
  put(ints, sizeof(ints));
  put(&pools, sizeof(pools));
  put(dims, sizeof(dims));
  for (int v : {RT_HDR_HORIZONTAL, RT_HDR_VERTICAL, RT_HDR_LLC_MINUS_CAMPOS, RT_HDR_CAMERA_LOCATION})
    put(h + 4 * v, 3 * sizeof(float));
  const float* sh = h + rt_off_shapes() / 4;
  for (int i = 0; i < nobj; ++i) {  // the sphere table's row i: the geometry, or NaN by the shape id
    put(sh + (size_t)i * 20, 4 * sizeof(float));
    put(sh + (size_t)i * 20 + 19, sizeof(float));
  }
  return n;
}

// Bounce-ray clusters of the AO kernel's later bounce rounds (rt_kernels_impl.h cluster_may_hit):
// the spheres among [0, nobj) are cut into spatial groups of at most max(kClusterSize, ceil(sqrt(nobj)))
// by recursive median splits of their centres along the widest axis (a round tests ~N/s balls and
// the members of the few it keeps: config (e), 256 spheres, AO 120.0 -> 116.0 ms per launch with
// groups of 16 instead of 8, 117.8 with 32; config (d), 64 spheres, 2.371 -> 2.395 ms with 16, so
// 8 there, profiles/r06s_*); each cluster is stored as (centre, R)
// with every member inside the ball: |c_i - centre| + |r_i| <= R (computed in double and
// rounded up).  Spheres that would inflate a cluster (radius above 8x the median, e.g. a ground
// sphere) and spheres with non-finite geometry are tested in every round instead (the always
// mask).  Non-spheres (NaN in the sphere table) are never accepted and are left out entirely.
// Returns the cluster count, 0 = off (small scenes, more than 256 objects, nothing to cluster).
constexpr int kClusterSize = 8;
constexpr int kClusterMinObj = 16;
int build_clusters(const Row* sph, int nobj, Row* ctab, unsigned long long* cmask) {
  std::memset(cmask, 0, sizeof(unsigned long long) * (1 + kMaxClusters) * kClusterWords);
  if (nobj < kClusterMinObj || nobj > 64 * kClusterWords) return 0;
  std::vector<int> small;
  std::vector<float> radii;
  for (int i = 0; i < nobj; ++i) {
    const Row g = sph[i];
    if (g.x != g.x) continue;  // not a sphere (NaN row): never accepted
    if (std::isfinite(g.x) && std::isfinite(g.y) && std::isfinite(g.z) && std::isfinite(g.w)) radii.push_back(std::fabs(g.w));
  }
  if (radii.size() < (size_t)kClusterSize) return 0;
  const int csize = std::max(kClusterSize, (int)std::ceil(std::sqrt((double)nobj)));
  std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
  const double big = 8.0 * radii[radii.size() / 2];
  for (int i = 0; i < nobj; ++i) {
    const Row g = sph[i];
    if (g.x != g.x) continue;
    const bool fin = std::isfinite(g.x) && std::isfinite(g.y) && std::isfinite(g.z) && std::isfinite(g.w);
    if (fin && std::fabs(g.w) <= big) small.push_back(i);
    else cmask[i >> 6] |= 1ull << (i & 63);  // always tested
  }
  // recursive median split into groups of <= csize
  std::vector<std::pair<int, int>> groups, work{{0, (int)small.size()}};
  while (!work.empty()) {
    auto [a, b] = work.back();
    work.pop_back();
    if (b - a <= csize) {
      groups.push_back({a, b});
      continue;
    }
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int k = a; k < b; ++k) {
      const Row g = sph[small[k]];
      const double v[3] = {g.x, g.y, g.z};
      for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], v[d]), hi[d] = std::max(hi[d], v[d]);
    }
    int ax = 0;
    for (int d = 1; d < 3; ++d)
      if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
    const int mid = (a + b) / 2;
    auto key = [&](int i) { const Row g = sph[i]; return ax == 0 ? g.x : ax == 1 ? g.y : g.z; };
    std::nth_element(small.begin() + a, small.begin() + mid, small.begin() + b,
                     [&](int i, int j) { return key(i) < key(j) || (key(i) == key(j) && i < j); });
    work.push_back({mid, b});
    work.push_back({a, mid});
  }
  if ((int)groups.size() > kMaxClusters) {  // too many groups: test everything every round
    std::memset(cmask, 0, sizeof(unsigned long long) * kClusterWords);
    return 0;
  }
  int k = 0;
  for (auto [a, b] : groups) {
    double cx = 0, cy = 0, cz = 0;
    for (int q = a; q < b; ++q) cx += sph[small[q]].x, cy += sph[small[q]].y, cz += sph[small[q]].z;
    const float fx = (float)(cx / (b - a)), fy = (float)(cy / (b - a)), fz = (float)(cz / (b - a));
    double R = 0.0;
    for (int q = a; q < b; ++q) {
      const Row g = sph[small[q]];
      const double dx = (double)g.x - fx, dy = (double)g.y - fy, dz = (double)g.z - fz;
      R = std::max(R, std::sqrt(dx * dx + dy * dy + dz * dz) + std::fabs((double)g.w));
      cmask[(size_t)(1 + k) * kClusterWords + (small[q] >> 6)] |= 1ull << (small[q] & 63);
    }
    ctab[k] = Row{fx, fy, fz, std::nextafter((float)(R * (1.0 + 1e-6)), INFINITY)};
    ++k;
  }
  return k;
}

// The ray queries' bounding-ball tree (include/rt/abi.h "Query tree"; the kernels: rt_kernels_impl.h
// ray_query_tree_kernel).  Members as build_clusters takes them: the spheres among [0, nobj) with
// finite geometry and |r| <= 8x the median |r|; the other spheres (a ground sphere, non-finite rows)
// go to the always list, which every ray tests; NaN rows (no sphere) are left out.  Recursive median
// splits of the members' centres along the widest axis, ties by index, down to leaves of at most
// kTreeLeaf; the nodes in preorder, each with the index of the next node that is not below it, so a
// traversal keeps no stack.  Every node stores a ball (centre, R):
//   leaf:   |c_i - centre| + |r_i| <= R for every member (centre: the mean of the members' centres),
//   inner:  |centre_child - centre| + R_child <= R for both children (centre and R: the smallest ball
//           around the children's two balls),
// R computed in binary64 from the stored binary32 centre and rounded up as build_clusters rounds its
// radius.  By the triangle inequality every sphere below a node lies inside the node's ball, which is
// all cluster_may_hit's proof asks of a ball.
namespace {

bool finite_row(const Row& g) { return std::isfinite(g.x) && std::isfinite(g.y) && std::isfinite(g.z) && std::isfinite(g.w); }
float round_up(double R) { return std::nextafter((float)(R * (1.0 + 1e-6)), INFINITY); }
double dist(const Row& a, double x, double y, double z) {
  const double dx = (double)a.x - x, dy = (double)a.y - y, dz = (double)a.z - z;
  return std::sqrt(dx * dx + dy * dy + dz * dz);
}

// the subtree over members m[a, b); returns its node
int tree_node(const Row* sph, std::vector<int>& m, int a, int b, QueryTreeHost& t) {
  const int k = (int)t.ball.size();
  t.ball.push_back(Row{});
  t.link.push_back(TreeLink{});
  if (b - a <= kTreeLeaf) {
    std::sort(m.begin() + a, m.begin() + b);
    double cx = 0, cy = 0, cz = 0;
    for (int q = a; q < b; ++q) cx += sph[m[q]].x, cy += sph[m[q]].y, cz += sph[m[q]].z;
    const float fx = (float)(cx / (b - a)), fy = (float)(cy / (b - a)), fz = (float)(cz / (b - a));
    double R = 0.0;
    const int first = (int)t.rows.size();
    for (int q = a; q < b; ++q) {
      const Row g = sph[m[q]];
      R = std::max(R, dist(g, fx, fy, fz) + std::fabs((double)g.w));
      t.rows.push_back(g);
      t.index.push_back(m[q]);
    }
    t.ball[k] = Row{fx, fy, fz, round_up(R)};
    t.link[k] = TreeLink{k + 1, first, b - a, 0};
    t.n_leaves += 1;
    return k;
  }
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int q = a; q < b; ++q) {
    const Row g = sph[m[q]];
    const double v[3] = {g.x, g.y, g.z};
    for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], v[d]), hi[d] = std::max(hi[d], v[d]);
  }
  int ax = 0;
  for (int d = 1; d < 3; ++d)
    if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
  const int mid = (a + b) / 2;
  auto key = [&](int i) { const Row g = sph[i]; return ax == 0 ? g.x : ax == 1 ? g.y : g.z; };
  std::nth_element(m.begin() + a, m.begin() + mid, m.begin() + b,
                   [&](int i, int j) { return key(i) < key(j) || (key(i) == key(j) && i < j); });
  const int l = tree_node(sph, m, a, mid, t);
  const int r = tree_node(sph, m, mid, b, t);
  // the smallest ball around the two children's: the larger one if it holds the other, else the
  // ball on the segment through both centres
  const Row A = t.ball[l], B = t.ball[r];
  const double d = dist(A, B.x, B.y, B.z);
  double cx, cy, cz;
  if (d + B.w <= A.w || !(d > 0.0)) cx = A.x, cy = A.y, cz = A.z;
  else if (d + A.w <= B.w) cx = B.x, cy = B.y, cz = B.z;
  else {
    const double s = 0.5 * (d + (double)B.w - (double)A.w) / d;  // from A's centre towards B's
    cx = A.x + s * ((double)B.x - A.x), cy = A.y + s * ((double)B.y - A.y), cz = A.z + s * ((double)B.z - A.z);
  }
  if (!(std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz))) cx = A.x, cy = A.y, cz = A.z;  // (R overflowed)
  const float fx = (float)cx, fy = (float)cy, fz = (float)cz;
  const double R = std::max(dist(A, fx, fy, fz) + (double)A.w, dist(B, fx, fy, fz) + (double)B.w);
  t.ball[k] = Row{fx, fy, fz, round_up(R)};
  t.link[k] = TreeLink{(int)t.ball.size(), 0, 0, 0};
  return k;
}

}  // namespace

void QueryTreeHost::reserve(int num_shapes) {
  const int n = num_shapes > 0 ? num_shapes : 0;
  ball.reserve(tree_max_nodes(n));
  link.reserve(tree_max_nodes(n));
  rows.reserve(n);
  index.reserve(n);
}

int build_query_tree(const Row* sph, int nobj, QueryTreeHost& t) {
  t.ball.clear();
  t.link.clear();
  t.rows.clear();
  t.index.clear();
  t.n_leaf_entries = t.n_always = t.n_leaves = 0;
  std::vector<float> radii;
  for (int i = 0; i < nobj; ++i)
    if (sph[i].x == sph[i].x && finite_row(sph[i])) radii.push_back(std::fabs(sph[i].w));
  if ((int)radii.size() < 2 * kTreeLeaf) return 0;
  std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
  const double big = 8.0 * radii[radii.size() / 2];
  std::vector<int> members, always;
  for (int i = 0; i < nobj; ++i) {
    const Row g = sph[i];
    if (g.x != g.x) continue;  // not a sphere (NaN row): never accepted
    if (finite_row(g) && std::fabs(g.w) <= big) members.push_back(i);
    else always.push_back(i);
  }
  if ((int)members.size() < 2 * kTreeLeaf) return 0;
  tree_node(sph, members, 0, (int)members.size(), t);
  t.n_leaf_entries = (int)t.rows.size();
  for (int i : always) {
    t.rows.push_back(sph[i]);
    t.index.push_back(i);
  }
  t.n_always = (int)always.size();
  return (int)t.ball.size();
}

int pack_header(const rt_config& cfg, const float* h, Row* tab, int& nobj, int& nplanes, int& ncl) {
  int nrects = 0;
  return pack_header(cfg, h, tab, nobj, nplanes, ncl, 0, nrects);
}

int pack_header(const rt_config& cfg, const float* h, Row* tab, int& nobj, int& nplanes, int& ncl, int flags,
                int& nrects) {
  const int S = cfg.num_shapes, spp = cfg.spp;
  const bool rects = (flags & RT_SCENE_RECTANGLES) != 0;
  int nr = 0;
  nobj = header_nobj(h, S);
  if (nobj < 0) return RT_E_INVAL;
  const float* sh = h + rt_off_shapes() / 4;
  const int Sc = table_stride(cfg);
  const float qnan = std::numeric_limits<float>::quiet_NaN();
  Row* sph = tab + sphere_table(Sc);
  Row* pln = tab + plane_table(Sc);
  int np = 0;
  for (int i = 0; i < S; ++i) {
    const float* s = sh + (size_t)i * 20;
    float idf = s[16 + 3];
    int id = (idf > -2147483648.0f && idf < 2147483648.0f) ? (int)idf : 0;  // int(simple_shapes[i][4].w)
    tab[i] = Row{s[0], s[1], s[2], s[3]};
    Row g2 = Row{s[12], s[13], s[14], 0.0f};
    std::memcpy(&g2.w, &id, 4);
    tab[(size_t)Sc + i] = g2;
    tab[(size_t)2 * Sc + i] = Row{s[16], s[17], s[18], s[19]};
    tab[(size_t)3 * Sc + i] = Row{s[4 + 3], s[12 + 3], 0.0f, 0.0f};
    // sphere table: the spheres' geometry; every other shape NaN (a NaN discriminant is never
    // accepted: eval_ray's -1 for shapes it does not intersect, p_compute.glsl:121-138).  A sphere
    // whose radius is NaN has a NaN discriminant on every ray, so sphere_eval_ray returns NaN and
    // neither a closest-hit scan nor a shadow ray ever takes it: it is packed as a NaN row too.  (With
    // its finite centre kept, sphere_eval_shadow's v_max_f32 clamp, which returns the other operand
    // for a NaN, went on with a root of 2^-50 and the sphere occluded what lay behind its centre.)
    sph[i] = id == RT_SHAPE_SPHERE && s[3] == s[3] ? tab[i] : Row{qnan, qnan, qnan, qnan};
    if (i < nobj && id == RT_SHAPE_PLANE) {  // plane table: (normal, bits(index)), (p0, 0)
      Row a = Row{s[0], s[1], s[2], 0.0f};
      std::memcpy(&a.w, &i, 4);
      pln[2 * np] = a;
      pln[2 * np + 1] = Row{s[12], s[13], s[14], 0.0f};
      ++np;
    } else if (rects && i < nobj && id == RT_SHAPE_RECTANGLE) {
      // a rectangle in effect: (n, bits(index)), (llc, bits(offset of its rows from the plane table));
      // the rows: (right, dot(right, right)), (up, dot(up, up)), the kernels' fused chain
      Row a = Row{s[0], s[1], s[2], 0.0f};
      std::memcpy(&a.w, &i, 4);
      Row b = Row{s[12], s[13], s[14], 0.0f};
      const int off = (int)(rect_table(Sc, spp) - plane_table(Sc)) + 2 * nr;
      std::memcpy(&b.w, &off, 4);
      pln[2 * np] = a;
      pln[2 * np + 1] = b;
      ++np;
      Row* rr = tab + rect_table(Sc, spp) + 2 * nr;
      rr[0] = Row{s[8], s[9], s[10], std::fmaf(s[10], s[10], std::fmaf(s[9], s[9], s[8] * s[8]))};
      rr[1] = Row{s[4], s[5], s[6], std::fmaf(s[6], s[6], std::fmaf(s[5], s[5], s[4] * s[4]))};
      ++nr;
    }
  }
  if (rects) std::memset((void*)(tab + rect_table(Sc, spp) + 2 * nr), 0, (size_t)(2 * Sc - 2 * nr) * sizeof(Row));
  nrects = nr;
  // the padding rows; the colour table's row -1 is the background (table_stride)
  for (int k = 0; k < 4; ++k) tab[(size_t)k * Sc + Sc - 1] = Row{0.0f, 0.0f, 0.0f, 0.0f};
  tab[4 * (size_t)Sc + Sc - 1] = Row{qnan, qnan, qnan, qnan};  // sphere table: never accepted
  {
    const float* bg = h + RT_HDR_BACKGROUND * 4;
    tab[(size_t)2 * Sc - 1] = Row{bg[0], bg[1], bg[2], bg[3]};
  }
  std::memcpy(tab + rand_table(Sc), h + rt_off_rand(S) / 4, (size_t)2 * spp * sizeof(Row));
  {  // camera-relative sphere rows: pmc = camera - centre, pp = dot(pmc, pmc) as the kernels'
    // sphere_candidate forms them (binary32, fmaf; this file is built with -ffp-contract=off)
    const float* cam = h + RT_HDR_CAMERA_LOCATION * 4;
    Row* crel = tab + camrel_table(Sc);
    for (int i = 0; i < Sc; ++i) {
      const Row g = sph[i];
      const float px = cam[0] - g.x, py = cam[1] - g.y, pz = cam[2] - g.z;
      crel[i] = Row{px, py, pz, std::fmaf(pz, pz, std::fmaf(py, py, px * px))};
    }
  }
  nplanes = np;
  ncl = build_clusters(sph, nobj, tab + cluster_table(Sc), (unsigned long long*)(tab + cluster_mask_table(Sc)));
  return RT_OK;
}

bool sched_order(int gx, int gy, int per_unit, const unsigned* cost, const std::vector<unsigned>& cur,
                 std::vector<unsigned>& next) {
  const int nunits = gx * gy;
  std::vector<unsigned> unit(nunits);
  for (int t = 0; t < nunits; ++t) {
    unsigned v = 0;
    for (int k = 0; k < per_unit; ++k) v = std::max(v, cost[(size_t)t * per_unit + k]);
    unit[t] = v;
  }
  next.resize(nunits);
  for (int t = 0; t < nunits; ++t) next[t] = (unsigned)t;
  std::stable_sort(next.begin(), next.end(), [&](unsigned a, unsigned b) { return unit[a] > unit[b]; });
  for (auto& t : next) t = (t % (unsigned)gx) | ((t / (unsigned)gx) << 16);  // packed x | y << 16
  const bool uniform = std::all_of(unit.begin(), unit.end(), [&](unsigned v) { return v == unit[0]; });
  return !uniform && next != cur;
}

int batch_slots(const unsigned char* same, int m, int prev, int nslots, int* slot) {
  int nd = 0;  // distinct new tables
  for (int j = 0; j < m; ++j) {
    if (same[j] && (j > 0 || prev >= 0)) slot[j] = j == 0 ? -1 : slot[j - 1];  // -1: the previous slot `prev`
    else slot[j] = -2 - nd++;                                                   // new table nd (its slot is fixed below)
  }
  // new tables go to slots base .. base + nd - 1, never over `prev` if frame 0 reads it
  const bool keep_prev = slot[0] == -1;
  const int base = keep_prev && prev + 1 + nd <= nslots ? prev + 1 : 0;
  for (int j = 0; j < m; ++j) slot[j] = slot[j] == -1 ? prev : base + (-2 - slot[j]);
  return base;
}

}  // namespace rt

extern "C" int rt_query_tree_host(const rt_config* cfg, const void* header, size_t header_bytes, int flags, float* balls,
                                  int32_t* links, int node_cap, float* leaf_rows, int32_t* leaf_index, int leaf_cap,
                                  int32_t* always, int always_cap, int* n_leaf, int* n_always) {
  if ((flags & ~RT_SCENE_RECTANGLES) != 0) return -1;
  if (!cfg || !header || !balls || !links || !leaf_rows || !leaf_index || !always || node_cap < 0 || leaf_cap < 0 ||
      always_cap < 0 || cfg->spp <= 0 || cfg->num_shapes < 0 ||
      header_bytes != rt_header_bytes(cfg->num_shapes, cfg->spp))
    return -1;
  // the table an upload packs (pack_header: the sphere table), then the tree over it
  const int Sc = rt::table_stride(*cfg);
  std::vector<rt::Row> tab(rt::table_vec4_rect(Sc, cfg->spp));
  int nobj = 0, np = 0, ncl = 0, nr = 0;
  if (rt::pack_header(*cfg, (const float*)header, tab.data(), nobj, np, ncl, flags, nr) != RT_OK) return -1;
  rt::QueryTreeHost t;
  const int n = rt::build_query_tree(tab.data() + rt::sphere_table(Sc), nobj, t);
  if (n > node_cap || t.n_leaf_entries > leaf_cap || t.n_always > always_cap) return -1;
  if (n_leaf) *n_leaf = t.n_leaf_entries;
  if (n_always) *n_always = t.n_always;
  if (n == 0) return 0;
  std::memcpy(balls, t.ball.data(), (size_t)n * sizeof(rt::Row));
  std::memcpy(links, t.link.data(), (size_t)n * sizeof(rt::TreeLink));
  std::memcpy(leaf_rows, t.rows.data(), (size_t)t.n_leaf_entries * sizeof(rt::Row));
  std::memcpy(leaf_index, t.index.data(), (size_t)t.n_leaf_entries * sizeof(int));
  std::memcpy(always, t.index.data() + t.n_leaf_entries, (size_t)t.n_always * sizeof(int));
  if (n_leaf) *n_leaf = t.n_leaf_entries;
  if (n_always) *n_always = t.n_always;
  return n;
}
