// The device copy of a backoff n-gram trie (pykaldi2_amd/ngram.py; made by pk2_ngram_create in lattice_lmrescore.hip): the one
// definition behind the opaque LM handle of include/pk2hip.h, shared by the kernels that look words up in it
// (lattice_lmrescore.hip, ctc_beam.hip).
#pragma once
#include <stdint.h>

namespace pk2 {

struct NgramDev {
  int32_t N = 0, order = 0, start = 0, eos = 0;
  void* blob = nullptr;
  const int32_t *d_word, *d_child, *d_bo, *d_next;
  const float *d_cost, *d_backoff;
};

}  // namespace pk2
