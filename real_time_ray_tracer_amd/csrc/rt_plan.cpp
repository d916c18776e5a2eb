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
    // accepted: eval_ray's -1 for shapes it does not intersect, p_compute.glsl:121-138)
    sph[i] = id == RT_SHAPE_SPHERE ? tab[i] : Row{qnan, qnan, qnan, qnan};
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
