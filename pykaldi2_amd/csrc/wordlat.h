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
  // word-boundary alignment (pk2_wordlat_set_strings, lattice_align_words.hip): the transition-id string of
  // every packed arc (offsets laid out like arc_off), per lattice the longest start -> end path in frames and the words of
  // alignment workspace in front of it; one device allocation of its own (null until set)
  std::vector<int32_t> fcap;
  std::vector<int64_t> align_pre;
  int32_t max_tid = 0;
  void* sblob = nullptr;
  const int64_t *d_tid_off = nullptr, *d_align_pre = nullptr;
  const int32_t *d_tids = nullptr, *d_fcap = nullptr;
  // system combination (pk2_wordlat_set_groups, lattice_combine.hip): the lattices are stored group by
  // group (one group = the systems' lattices of one utterance).  Host copies for validation and workspace sizes, one
  // device allocation of its own (null until set).  est_pre: words of E-step workspace in front of every lattice, rows
  // sized by its GROUP's capacity; grp_pre / gpe_pre: words of Gamma and state, and even row lengths, in front of every group.
  std::vector<int32_t> h_word_ids;      // laid out like d_word_ids
  int NG = 0;
  std::vector<int32_t> group_off, gcap;
  std::vector<int64_t> est_pre, grp_pre, gpe_pre;
  void* gblob = nullptr;
  const int32_t *d_group_off, *d_lat_group, *d_gcap, *d_uvoc, *d_map;
  const double *d_wn, *d_logwn;
  const int64_t *d_uvoc_off, *d_map_off, *d_est_pre, *d_grp_pre, *d_gpe_pre;
};

}  // namespace pk2
