// Forced alignment: what the host compiler (csrc/align_graph.hip) hands the device Viterbi (csrc/align_viterbi.hip).
//
// One packed int32 buffer per minibatch: N descriptors (AlignDesc, 16 words each), then per utterance its arrays,
// each starting on a 16-word boundary; the descriptor's fields are word offsets into the buffer.  Per utterance:
//   in_off[S+1]       in-arcs of state s are in_off[s] .. in_off[s+1]
//   arcx[A]           (src + 1) << 1 | self_loop   (src = -1: the arc leaves the start state; only frame 0 uses it)
//   w[A]  f32         graph cost of the arc
//   tid[A], pdf[A]    transition-id and its pdf
//   fpdf[S], lpdf[S]  pdf of the non-self-loop in-arcs / of the self-loop of state s (every arc into s is one of the two)
//   fin[S] f32        final cost, +inf when s is not final
// bp / scr are byte offsets into the caller's workspace: bp = u32[T][S] backpointers, scr = f32[2 S] (per-frame costs
// when they do not live in LDS) followed by f32[2 T] (graph / acoustic cost of the chosen arc per frame).
#pragma once
#include <cstdint>

namespace pk2 {

struct AlignDesc {
  int32_t S, A, T, status;   // status: 0 = compiled, 2 = no path of T frames (S = A = 0 then)
  int32_t in_off, arcx, w, tid, pdf, fpdf, lpdf, fin;
  int64_t bp, scr;
};
static_assert(sizeof(AlignDesc) == 64, "AlignDesc is 16 words");

constexpr int kAlignThreads = 512;
constexpr int kAlignMaxStates = 32 * kAlignThreads;   // 16 bits of a backpointer hold src + 1; SPT <= 32

}  // namespace pk2
