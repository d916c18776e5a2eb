// rt_tree.hip — the ray queries' tree on the device (rt_tree.h).
#include "rt_tree.h"

#include <cstring>

namespace rt {

namespace {

static_assert(sizeof(TreeLink) == sizeof(float4) && sizeof(Row) == sizeof(float4), "a node is two float4");

// One upload's layout: 2 n float4 of nodes, e float4 of rows, e ints, for n nodes and e entries.
size_t image_bytes(size_t nodes, size_t entries) { return nodes * 2 * sizeof(float4) + entries * (sizeof(float4) + sizeof(int)); }

}  // namespace

size_t QueryTreeState::buffer_bytes(int num_shapes) {
  const int n = num_shapes > 0 ? num_shapes : 0;
  const size_t b = image_bytes((size_t)tree_max_nodes(n), (size_t)n);
  return b > 0 ? b : 16;
}

int QueryTreeState::enable(int num_shapes, int& last_hip) {
  if (on) return RT_OK;
  const size_t need = buffer_bytes(num_shapes);
  int rc = alloc_or_nomem(&d_buf, need, last_hip);
  if (rc != RT_OK) return rc;
  bytes = need;
  cap = num_shapes > 0 ? num_shapes : 0;
  host.reserve(cap);
  key.reserve(sizeof(int) + (size_t)cap * sizeof(Row));
  image.reserve(need);
  on = true;
  have_key = false;
  n_nodes = 0;
  return RT_OK;
}

int QueryTreeState::update(const Row* sph, int nobj, StageRing& stage, hipStream_t st, int& last_hip) {
  if (!on) return RT_OK;
  if (nobj < 0 || nobj > cap) return RT_E_INVAL;  // (never: the header was checked against num_shapes)
  const size_t kb = sizeof(int) + (size_t)nobj * sizeof(Row);
  if (have_key && key.size() == kb && std::memcmp(key.data(), &nobj, sizeof(int)) == 0 &&
      (nobj == 0 || std::memcmp(key.data() + sizeof(int), sph, (size_t)nobj * sizeof(Row)) == 0))
    return RT_OK;
  key.resize(kb);
  std::memcpy(key.data(), &nobj, sizeof(int));
  if (nobj > 0) std::memcpy(key.data() + sizeof(int), sph, (size_t)nobj * sizeof(Row));
  have_key = true;
  n_nodes = build_query_tree(sph, nobj, host);
  builds += 1;
  if (n_nodes == 0) return RT_OK;
  const size_t e = host.rows.size();
  const size_t nb = (size_t)n_nodes * 2 * sizeof(float4), rb = e * sizeof(float4), ib = e * sizeof(int);
  if (nb + rb + ib > bytes) return RT_E_INVAL;  // (never: tree_max_nodes bounds the build)
  image.resize(nb + rb + ib);
  for (int k = 0; k < n_nodes; ++k) {  // a node: its ball, then its link
    std::memcpy(image.data() + (size_t)k * 2 * sizeof(float4), &host.ball[k], sizeof(float4));
    std::memcpy(image.data() + ((size_t)k * 2 + 1) * sizeof(float4), &host.link[k], sizeof(float4));
  }
  std::memcpy(image.data() + nb, host.rows.data(), rb);
  std::memcpy(image.data() + nb + rb, host.index.data(), ib);
  return stage.copy(d_buf, image.data(), image.size(), st, last_hip);
}

const QueryTree* QueryTreeState::view(QueryTree& v) const {
  if (!on || n_nodes == 0) return nullptr;
  const size_t e = host.rows.size();
  v.nodes = (const float4*)d_buf;
  v.rows = v.nodes + (size_t)2 * n_nodes;
  v.index = (const int*)(v.rows + e);
  v.n_nodes = n_nodes;
  v.always_first = host.n_leaf_entries;
  v.n_always = host.n_always;
  return &v;
}

void QueryTreeState::release() {
  if (d_buf) (void)hipFree(d_buf);
  *this = QueryTreeState{};
}

}  // namespace rt
