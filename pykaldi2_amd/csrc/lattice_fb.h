// What the lattice forward-backward (lattice_fb.hip) shares with the kernels that rescore a lattice between two of its
// runs (lattice_rescore.hip): the parameter block, the per-utterance view of the workspace, a link's scaled
// log-likelihood, and the host-side launches of the recursions and of the plain posterior pass.
#pragma once
#include <cmath>

#include "lattice_internal.h"

namespace pk2 {

constexpr int kFbThreads = 1024;
constexpr int kFbWaves = kFbThreads / 64;

template <typename T>
__device__ __forceinline__ T ldc(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct FbParams {
  LatPtrs L;
  const int32_t* ref_tids; int64_t ref_stride;
  const int32_t* tid2pdf; const int32_t* tid2phone; const uint8_t* phone_sil;
  int32_t criterion, one_silence_class, drop_frames;
  double lm_scale, ac_scale;
  float* post; int64_t post_seq_stride, post_frame_stride;
  double* out;   // [N] lat_like (MMI, plain posteriors) or expected accuracy (MPE)
  float post_sign;   // plain posteriors: post += post_sign * gamma
};

__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < kFbWaves; ++k) r += red[k];
  return r;
}

// Per-utterance views shared by the kernels.
struct FbView {
  int T, nt;
  const int32_t* ftok; const int32_t* seg; const int32_t* kept; const int32_t* maxlev;
  const int4* lrec; const float* lac; const int32_t* tl; const float* tf;
  double* alpha; double* beta; double* af; double* ab;
  const int32_t* ref; double* ref_post;
  LatFrame* F;
  double* lw; double* sca; double* scb;       // linear-domain recursion: link weights, per-frame log scales of alpha / beta
};
__device__ __forceinline__ FbView fb_view(const FbParams& p, int n, const LatUtt& U) {
  FbView v;
  v.T = U.T; v.nt = U.n_tok;
  v.ftok = p.L.frame_tok + U.frame_base; v.seg = p.L.seg_off + U.frame_base;
  v.kept = p.L.seg_kept + U.frame_base; v.maxlev = p.L.frame_maxlev + U.frame_base;
  v.lrec = p.L.link_rec + U.link_base;      // {src token, dst token, transition-id, graph cost bits}
  v.lac = p.L.link_ac + U.link_base;
  v.tl = p.L.tok_level + U.tok_base; v.tf = p.L.tok_final + U.tok_base;
  v.alpha = p.L.alpha + U.tok_base; v.beta = p.L.beta + U.tok_base;
  v.af = p.L.acc_f + U.tok_base; v.ab = p.L.acc_b + U.tok_base;
  v.ref = p.ref_tids ? p.ref_tids + (int64_t)n * p.ref_stride : nullptr;      // (null: the plain posteriors have no reference)
  v.ref_post = p.L.ref_post + U.frame_base;
  v.F = p.L.frame + n;
  v.lw = p.L.link_w + U.link_base; v.sca = p.L.fb_scale + U.frame_base; v.scb = p.L.fb_scale + p.L.frame_total + U.frame_base;
  return v;
}
// fst::ScaleLattice stores the scaled weights as floats; the forward-backward then sums them in double
__device__ __forceinline__ double scaled_like(const FbParams& p, float graph, float ac) {
  return -((double)(float)(p.lm_scale * (double)graph) + (double)(float)(p.ac_scale * (double)ac));
}
__device__ __forceinline__ double link_like(const FbParams& p, const FbView& v, const int4& r, int l) {
  return scaled_like(p, __int_as_float(r.w), v.lac[l]);
}
__device__ __forceinline__ double final_like(const FbParams& p, const FbView& v, int i) {
  return -(double)(float)(p.lm_scale * (double)v.tf[i]);
}

// linear value x at log scale r -> its log (r is NaN when x is a log already; -inf marks a token nothing reaches)
__device__ __forceinline__ double fb_log_of(double x, double r) { return (r == r && x != -INFINITY) ? r + log(x) : x; }

// Host side (lattice_fb.hip).  fb_recursions: alpha / beta of every utterance under p's scales and the total
// log-likelihood in the utterance's frame state (failed utterances: p.out[n] = NaN); with_acc also clears the accuracy
// accumulators of sMBR / MPFE.  *linear: the values lie in memory as the linear-domain kernel leaves them (fb_log_of with
// fb_scale reads them; a recursion that left the linear form's range has been run again in the log domain, its frame scales say
// "logs").  fb_plain_posteriors: post += post_sign * gamma per (frame, pdf), p.out[n] = the total (NaN when it is not finite).
int fb_recursions(const pk2_lattice_batch* b, const FbParams& p, int with_acc, hipStream_t stream, bool* linear);
int fb_plain_posteriors(const pk2_lattice_batch* b, const FbParams& p, bool linear, hipStream_t stream);

}  // namespace pk2
