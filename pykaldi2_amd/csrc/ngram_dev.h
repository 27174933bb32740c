// The device copy of a backoff n-gram trie (pykaldi2_amd/ngram.py; made by pk2_ngram_create in lattice_lmrescore.hip): the one
// definition behind the opaque LM handle of include/pk2hip.h, and the one arc lookup of the kernels that look words up in it
// (lattice_lmrescore.hip, ctc_beam.hip).
#pragma once
#include "common.h"

namespace pk2 {

struct NgramDev {
  int32_t N = 0, order = 0, start = 0, eos = 0;
  void* blob = nullptr;
  const int32_t *d_word, *d_child, *d_bo, *d_next;
  const float *d_cost, *d_backoff;
};

// The six device arrays of the trie, as a kernel's parameter block carries them.
struct NgramTrie {
  const int32_t *word, *child, *bo, *next;
  const float *cost, *backoff;
};
inline NgramTrie ngram_trie(const NgramDev& lm) { return NgramTrie{lm.d_word, lm.d_child, lm.d_bo, lm.d_next, lm.d_cost, lm.d_backoff}; }

// cost and next state of word w from LM state h (arc(h, w)): the float64 sum of float32 trie entries along
// the backoff chain; false if w has no unigram
__device__ __forceinline__ bool ngram_arc(const NgramTrie& g, int h, int w, double& cost, int& next) {
  double acc = 0.0;
  int node = h;
#pragma nounroll
  for (int it = 0; it <= PK2_NGRAM_MAX_ORDER; ++it) {
    const int end = g.child[node + 1];
    int lo = g.child[node], hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (g.word[mid] < w) lo = mid + 1; else hi = mid;
    }
    if (lo < end && g.word[lo] == w) { cost = acc + (double)g.cost[lo]; next = g.next[lo]; return true; }
    if (node == 0) break;
    acc += (double)g.backoff[node];
    node = g.bo[node];
  }
  cost = 0.0; next = 0;
  return false;
}

}  // namespace pk2
