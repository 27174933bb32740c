// Full-sum numerator over training graphs (csrc/chain_num_graph.hip), as csrc/chain_objf.hip calls it.
#pragma once
#include "common.h"

struct pk2_align_graphs;

namespace pk2 {

size_t num_graph_workspace(const pk2_align_graphs* G);
int num_graph_use_lds(const pk2_align_graphs* G);
// Adds scale * posterior into grad rows t < T of every compiled utterance; logprob[n] = log p_num, status[n] as compiled
// (an utterance without a graph gets logprob 0 and its rows are left alone).  workspace: 256-byte aligned.
int num_graph_compute(const pk2_align_graphs* G, const int32_t* packed_dev, const float* logits, int64_t seq_stride,
                      int64_t frame_stride, int32_t num_pdfs, float scale, float* grad, int64_t gss, int64_t gfs, float* logprob,
                      int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t stream);

}  // namespace pk2
