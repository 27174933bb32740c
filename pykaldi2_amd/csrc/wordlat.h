// The uploaded batch of packed word lattices (pk2_wordlat_create, lattice_score.hip), shared by the scoring kernels and the
// LM rescoring kernel (lattice_lmrescore.hip).  Every index in it was validated on the host.
#pragma once
#include <cstdint>
#include <vector>

namespace pk2 {

struct WordLat {
  int N = 0;
  std::vector<int64_t> state_off, arc_off, level_off_off, word_off_off, post_pre, mbr_pre, pe_pre;
  std::vector<int32_t> depth, cap;
  void* blob = nullptr;
  const int64_t *d_state_off, *d_arc_off, *d_level_off_off, *d_word_off_off, *d_post_pre, *d_mbr_pre, *d_pe_pre;
  const int32_t *d_src, *d_dst, *d_word, *d_in_off, *d_out_off, *d_out_idx, *d_level_off, *d_word_ids, *d_word_off, *d_word_arcs;
  const float *d_graph, *d_acoustic;
  // word times (pk2_wordlat_set_times): host copies of the arc endpoints for its validation, and the
  // frame at which every state is reached, laid out like state_off (a device allocation of its own, null until set)
  std::vector<int32_t> h_src, h_dst;
  int32_t* d_state_time = nullptr;
};

}  // namespace pk2
