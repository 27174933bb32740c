// The chain model as the host-side graph builders see it (csrc/chain_sup.hip, csrc/align_graph.hip): HMM topologies,
// the tuples of the transition model and the flattened context-dependency tree (layout: include/pk2hip.h,
// pk2_sup_model_create).
#pragma once
#include <algorithm>
#include <array>
#include <set>
#include <vector>

#include "common.h"

struct pk2_sup_model {
  int32_t N = 0, P = 0;
  std::vector<int32_t> phone2entry, entry_off, fwd_class, loop_class, trans_off, trans_dst;
  std::vector<int32_t> kind, key, a, b, pool;
  std::set<std::array<int32_t, 4>> tuples;
};

namespace pk2 {

// EventMap::Map on the flattened tree.
inline bool tree_answer(const pk2_sup_model& m, const int32_t* window, int32_t pdf_class, int32_t* ans) {
  int32_t node = 0;
  for (size_t guard = 0; guard <= m.kind.size(); ++guard) {
    if (node < 0 || node >= (int32_t)m.kind.size()) return false;
    if (m.kind[node] == 0) { *ans = m.a[node]; return true; }
    const int32_t k = m.key[node];
    if (k < -1 || k >= m.N) return false;
    const int32_t v = k == -1 ? pdf_class : window[k];
    const int32_t* p = m.pool.data() + m.a[node];
    if (m.kind[node] == 1) {
      if (v < 0 || v >= m.b[node]) return false;
      node = p[v];
    } else {
      node = p[m.b[node] + (std::binary_search(p, p + m.b[node], v) ? 0 : 1)];
    }
  }
  return false;   // cycle in a malformed tree
}

}  // namespace pk2
