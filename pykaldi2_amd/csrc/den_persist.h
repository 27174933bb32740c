// Persistent denominator recursion (chain_den_persist2.hip): internal interface used by chain_den.hip.
#pragma once
#include <vector>

#include "den_kernels.h"

namespace pk2 {

constexpr int kMaxTeams = 8;                         // teams per XCD the control block has room for
constexpr int kMaxTasks = 64;

// Chunked LDS table, two resident passes, streamed overflow -- any graph whose ranks hold at most kPMaxRows rows and whose
// vector needs at most kMaxChunks table chunks.
constexpr size_t kDenPersist2MaxLds = 160 * 1024 - 256;
// LDS of a workgroup: the table, seven row arrays of `cap` floats (sums of pass A, of pass B, of the streamed segments, x
// of own rows, two per-row constants, and the two 16-bit compact-row maps), and the small fixed part (reduction scratch,
// the segments' wave carries and their rows, flags).
constexpr int kP2RowArrays = 8;      // (the eighth: the pdfs of own rows and own states as shorts, round 4 -- left out, with
                                     // the x gather, for a graph it would cost a table chunk: pk2_den_graph::p2_rowarrays)
constexpr int kP2FixedFloats = 2 * kPW + 4 + 2 * kSegs * kPW + 16;
inline size_t den_persist2_lds_bytes(int tfloats, int cap, int arrays = kP2RowArrays) {
  return ((size_t)tfloats + arrays * (size_t)cap + kP2FixedFloats) * sizeof(float);
}
// The layouts exist and the LDS need fits a workgroup (a property of the graph alone).
bool den_persist2_fits(const pk2_den_graph* g);
// ... and no earlier launch has failed its verification on this device.  Whether a call uses the kernel is den_plan's
// decision (chain_den.hip).
bool den_persist2_usable(const pk2_den_graph* g);
// Runs the forward and backward recursions of all N sequences (one group per sequence; `p` as the launch-per-frame kernels
// would receive it, `xv` = [G][Tmax][V] exp(logit) per virtual state).  Leaves alpha, alphav, apart, asum, the btilde' slots
// of `beta` and bpart where den_step_sx<1> leaves them, with kPR partial sums per frame (bpart: shares whose sum over the
// ranks is the frame's sum, not sums over a rank's own states).  *ran = false when the device failed the first-use
// verification (the caller then replays the frame launches).
// `tail`: the minibatch's deferred numerator forward-backward (may be null); *num_ran = true when it rode in this launch
// (as tasks behind the recursions) and must not be launched again; num_ran = null: it may not ride.
struct NumDeferred;
int den_persist2_launch(pk2_den_graph* g, const DenParams& p, const float* xv, const int32_t* lengths_host, int N,
                        hipStream_t stream, bool* ran, const NumDeferred* tail = nullptr, bool* num_ran = nullptr,
                        bool xgather = false);      // xgather: `xv` is exp(logits) [G][Tmax][P], gathered by pdf
void den_persist2_check_launch(float* den_lp, int N, hipStream_t stream);
// Round 6: the check as a phase of den_tail1 (chain_den.hip) instead of a launch of its own.  Fills `ck` from the scratch of the
// persistent launch that has just run on `stream` (false: there was none) and books the control block as zeroed.
struct DenTailCheck { unsigned* ctl; int ctl_words; int ntasks; unsigned* abort_word; unsigned* done_word; unsigned* count_word;
                      unsigned* guard_dev; unsigned* guard_host; };
bool den_persist2_tail_check(hipStream_t stream, DenTailCheck* ck);

// Scratch of the launches on one (device, stream): the control block, the parameter block, the exchange words and
// the ring of state vectors, which grows with the graphs it has served.
struct DenPersistCtl;
struct DenPersistScratch {
  void* params = nullptr; DenPersistCtl* ctl = nullptr; float* ring = nullptr; float* pring = nullptr; int rpad = 0;
  int ntasks = 0;                             // recursions of the last launch that passed (what its check kernel expects)
  bool ctl_clean = false;                     // the last launch's check has zeroed the control block
  std::vector<unsigned char> params_host;     // what `params` holds (a call with the same block skips the store)
};

}  // namespace pk2
