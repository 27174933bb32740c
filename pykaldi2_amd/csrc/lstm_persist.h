// Persistent LSTM recurrences (lstm_persist_seq.hip, lstm_persist_big.hip): internal interface used by lstm.hip.
#pragma once
#include "common.h"

namespace pk2 {

// One (sequence, direction) per XCD (lstm_persist_seq.hip): the tensors and layouts of the step kernels, one launch per
// layer.  *ran = false when the persistent path is unusable on this device (checked once by the forward pass): the caller
// then uses the step kernels.
bool lstm_seq_wanted(int B, int H, int D);
int lstm_fwd_seq_launch(const float* gx, const float* whh, const float* bhh, int B, int T, int H, int D, float* y,
                        float* gates, float* cells, hipStream_t stream, bool* ran);
// The same launch computing its own input projections gx = inp W_ih^T + b_ih (lstm_fwd_seq2_xproj): inp [T][B][in_size],
// wih [D][4H][in_size], bih [D][4H] or null.  *ran = false: not fused (PK2_LSTM_SEQ_XPROJ, more than 8 pairs, in_size,
// alignment, residency, a device not verified yet) -- nothing was launched or written, the caller multiplies and calls
// lstm_fwd_seq_launch.
int lstm_fwd_seq_xproj_launch(const float* inp, int in_size, const float* wih, const float* bih, const float* whh, const float* bhh,
                              int B, int T, int H, int D, float* y, float* gates, float* cells, hipStream_t stream, bool* ran);
// dbias_ih / dbias_hh (may be null): [D][4H] accumulators (+=) of the bias gradient, filled by the kernel inside its
// launch; *bias_done says whether it was.
// wgrad (may be null): the recurrent weight gradient from inside the recurrence -- y [T][B][D*H] the forward pass's
// output, dwhh [D][4H][H] accumulated into (+=), ws at least lstm_seq_wgrad_workspace_floats(B, H, D) floats; done says
// whether dwhh has received it (false: dwhh and ws untouched).
struct SeqWgradCall { const float* y; float* dwhh; float* ws; bool done; };
size_t lstm_seq_wgrad_workspace_floats(int B, int H, int D);
int lstm_bwd_seq_launch(const float* dy, const float* whh, const float* gates, const float* cells, int B, int T, int H,
                        int D, float* dgx, hipStream_t stream, bool* ran, float* dbias_ih = nullptr, float* dbias_hh = nullptr,
                        bool* bias_done = nullptr, SeqWgradCall* wgrad = nullptr);
int lstm_seq_status(unsigned* abort_flag);

// Large batches (B >= 32, H = 512; lstm_persist_big.hip): a (direction, 64-row batch tile) task per XCD team, the rank's
// W_hh slice resident in LDS, one launch per layer.
bool lstm_big_wanted(int B, int H, int D);
int lstm_fwd_big_launch(const float* gx, const float* whh, const float* bhh, int B, int T, int H, int D, float* y,
                        float* gates, float* cells, hipStream_t stream, bool* ran);
// *all_gather: which of the two backward forms was launched (lstm_bwd_big_persist, not lstm_bwd_big_persist2).
int lstm_bwd_big_launch(const float* dy, const float* whh, const float* gates, const float* cells, int B, int T, int H,
                        int D, float* dgx, hipStream_t stream, bool* ran, bool* all_gather);
int lstm_big_status(unsigned* abort_flag);

}  // namespace pk2
