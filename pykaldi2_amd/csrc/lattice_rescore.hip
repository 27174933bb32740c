// Rescoring of the device lattices and the lattice teacher-student criterion (ops.TeacherStudentMMI; the reference's
// ops/ops.py:77-117 with its loss made well-defined).
//
//   pk2_lattice_rescore   Kaldi's RescoreLattice on the raw state-level lattices lattice_decode.hip left in the workspace: the
//                         acoustic cost of every kept emitting link t -> t+1 becomes
//                           old_acoustic_scale * cost - loglikes[t][tid2pdf[tid]]      (two float roundings; scale 0: -loglike)
//                         Epsilon links, tokens, link records, final costs, segments and the pruning result stay as they are.
//   pk2_lattice_ts        forward-backward with the lattice's own (teacher) scores; ONE pass over the kept emitting links that
//                         takes gamma_T, adds -gamma_T to the gradient, sums gamma_T (like_T - like_S) per utterance and writes
//                         the rescored cost in place (a link belongs to exactly one thread); forward-backward again; +gamma_S
//                         into the same gradient buffer; loss = sum gamma_T (like_T - like_S) - tot_T + tot_S = KL(P_T || P_S)
//                         over the paths of the lattice.  Nothing crosses to the host.
//
// This file is compiled with -ffp-contract=off (pykaldi2_amd/build.py): the rescoring rule is two separate float operations.
#include <cmath>

#include "lattice_fb.h"

namespace pk2 {

struct RescoreParams {
  const float* ll; int64_t seq_stride, frame_stride;      // loglikes[n][t][pdf] at n seq_stride + t frame_stride + pdf
  int32_t num_pdfs, num_tids;
  float old_scale;
  double* loss; double* like_T; double* like_S;           // teacher-student only
};

// pdf of a link's transition-id, -1 when the table does not cover it (such a link gets cost +inf: no path takes it)
__device__ __forceinline__ int rescore_pdf(const RescoreParams& s, const int32_t* tid2pdf, int tid) {
  const int pdf = (tid >= 1 && tid <= s.num_tids) ? tid2pdf[tid] : -1;
  return (pdf >= 0 && pdf < s.num_pdfs) ? pdf : -1;
}
__device__ __forceinline__ float rescored_cost(const RescoreParams& s, const float* rows, int t, int pdf, float old_ac) {
  if (pdf < 0) return INFINITY;
  const float x = rows[(int64_t)t * s.frame_stride + pdf];
  if (s.old_scale == 0.f) return -x;
  const float kept = s.old_scale * old_ac;
  return kept - x;
}

// The kept emitting links by segment, frames dealt round-robin to the workgroups of an utterance (as lat_fb_prep walks them).
__global__ void __launch_bounds__(256) lat_rescore(FbParams p, RescoreParams s) {
  const int n = blockIdx.y;
  const LatUtt U = p.L.utt[n];
  if (U.status != kLatOk) return;
  const FbView v = fb_view(p, n, U);
  float* lac = p.L.link_ac + U.link_base;
  const float* rows = s.ll + (int64_t)n * s.seq_stride;
  for (int t = blockIdx.x; t < v.T; t += gridDim.x) {
    const int m0 = v.seg[2 * t + 1], m1 = m0 + v.kept[2 * t + 1];
    for (int l = m0 + threadIdx.x; l < m1; l += 256)
      lac[l] = rescored_cost(s, rows, t, rescore_pdf(s, p.tid2pdf, v.lrec[l].z), lac[l]);
  }
}

// Between the teacher's and the student's forward-backward (geometry of lat_fb_posteriors): gamma_T of every kept emitting
// link from the alpha / beta in memory, -gamma_T into the gradient, gamma_T (like_T - like_S) summed per workgroup in double
// (one atomic per workgroup), and the link's rescored cost written over the teacher's.
__global__ void __launch_bounds__(kFbThreads) lat_ts_pass(FbParams p, RescoreParams s, int lin) {
  __shared__ double red[kFbWaves];
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const int n = blockIdx.y, tid = threadIdx.x;
  const LatUtt U = p.L.utt[n];
  if (U.status != kLatOk) return;
  const FbView v = fb_view(p, n, U);
  const double tot = v.F->fb_tot;
  if (blockIdx.x == 0 && tid == 0) s.like_T[n] = tot;
  const bool ok = fabs(tot) < INFINITY;
  float* lac = p.L.link_ac + U.link_base;
  const float* rows = s.ll + (int64_t)n * s.seq_stride;
  float* grad = p.post + (int64_t)n * p.post_seq_stride;
  double acc = 0.0;
  for (int t = blockIdx.x; t < v.T; t += gridDim.x) {
    const int m0 = v.seg[2 * t + 1], m1 = m0 + v.kept[2 * t + 1];
    const double ra = lin ? v.sca[t] : kNaN, rb = lin ? v.scb[t + 1] : kNaN;
    float* row = grad + (int64_t)t * p.post_frame_stride;
    for (int l = m0 + tid; l < m1; l += kFbThreads) {
      const int4 q = v.lrec[l];
      const int pdf = rescore_pdf(s, p.tid2pdf, q.z);
      const float old_ac = lac[l], new_ac = rescored_cost(s, rows, t, pdf, old_ac);
      if (ok && pdf >= 0) {
        const float graph = __int_as_float(q.w);
        const double like_T = scaled_like(p, graph, old_ac);
        const double g = exp(fb_log_of(v.alpha[q.x], ra) + like_T + fb_log_of(v.beta[q.y], rb) - tot);
        if (g > 0.0) {
          atomicAdd(&row[pdf], -(float)g);
          acc += g * (like_T - scaled_like(p, graph, new_ac));
        }
      }
      lac[l] = new_ac;
    }
  }
  acc = block_sum_d(acc, red);
  if (tid == 0 && acc != 0.0) atomicAdd(&s.loss[n], acc);
}

// loss = sum gamma_T (like_T - like_S) - tot_T + tot_S; an utterance whose lattice (decoded, or rescored) has no path of
// non-zero weight gets NaN and an all-zero gradient block.
__global__ void __launch_bounds__(256) lat_ts_finish(FbParams p, RescoreParams s) {
  const int n = blockIdx.y;
  const LatUtt U = p.L.utt[n];
  const double tot_T = s.like_T[n], tot_S = s.like_S[n];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (U.status == kLatOk && fabs(tot_T) < INFINITY && fabs(tot_S) < INFINITY) {
    if (first) s.loss[n] = s.loss[n] - tot_T + tot_S;
    return;
  }
  if (first) s.loss[n] = NAN;
  float* grad = p.post + (int64_t)n * p.post_seq_stride;
  const int64_t cells = (int64_t)U.T * s.num_pdfs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256)
    grad[(i / s.num_pdfs) * p.post_frame_stride + i % s.num_pdfs] = 0.f;
}

}  // namespace pk2

using namespace pk2;

static int rescore_args(const char* who, const pk2_lattice_batch* b, const void* workspace, const float* loglikes,
                        int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids) {
  PK2_REQUIRE(b && workspace && loglikes && tid2pdf, "%s: null pointer", who);
  PK2_REQUIRE(b->decoded, "%s: pk2_lattice_decode has not run on this batch", who);
  PK2_REQUIRE(num_pdfs > 0 && num_pdfs == b->num_pdfs, "%s: num_pdfs %d, but the batch was decoded with %d", who, num_pdfs,
              b->num_pdfs);
  PK2_REQUIRE(num_tids >= b->graph->max_ilabel, "%s: HCLG uses transition-id %d but the model has %d", who,
              b->graph->max_ilabel, num_tids);
  return PK2_OK;
}

extern "C" int pk2_lattice_rescore(const pk2_lattice_batch* b, void* workspace, const float* loglikes, int64_t seq_stride,
                                   int64_t frame_stride, int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids,
                                   float old_acoustic_scale, void* stream_) {
  int rc = rescore_args("lattice rescore", b, workspace, loglikes, num_pdfs, tid2pdf, num_tids);
  if (rc) return rc;
  FbParams p{};
  lattice_carve(b, workspace, &p.L);
  p.tid2pdf = tid2pdf;
  RescoreParams s{};
  s.ll = loglikes; s.seq_stride = seq_stride; s.frame_stride = frame_stride; s.num_pdfs = num_pdfs; s.num_tids = num_tids;
  s.old_scale = old_acoustic_scale;
  hipLaunchKernelGGL(lat_rescore, dim3(256, b->N), dim3(256), 0, static_cast<hipStream_t>(stream_), p, s);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_lattice_ts(const pk2_lattice_batch* b, void* workspace, const float* loglikes_S, int64_t seq_stride,
                              int64_t frame_stride, int32_t num_pdfs, const int32_t* tid2pdf, int32_t num_tids,
                              float old_acoustic_scale, double lm_scale, double acoustic_scale, float* grad,
                              int64_t grad_seq_stride, int64_t grad_frame_stride, double* loss, double* like_T,
                              double* like_S, void* stream_) {
  int rc = rescore_args("lattice teacher-student", b, workspace, loglikes_S, num_pdfs, tid2pdf, num_tids);
  if (rc) return rc;
  PK2_REQUIRE(grad && loss && like_T && like_S, "lattice teacher-student: null output");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FbParams p{};
  lattice_carve(b, workspace, &p.L);
  p.tid2pdf = tid2pdf; p.lm_scale = lm_scale; p.ac_scale = acoustic_scale; p.post_sign = 1.f;
  p.post = grad; p.post_seq_stride = grad_seq_stride; p.post_frame_stride = grad_frame_stride;
  RescoreParams s{};
  s.ll = loglikes_S; s.seq_stride = seq_stride; s.frame_stride = frame_stride; s.num_pdfs = num_pdfs; s.num_tids = num_tids;
  s.old_scale = old_acoustic_scale; s.loss = loss; s.like_T = like_T; s.like_S = like_S;
  PK2_HIP(hipMemsetAsync(loss, 0, sizeof(double) * b->N, stream));
  bool linear = false;
  p.out = like_T;                                   // (a failed utterance gets its NaN here)
  if ((rc = fb_recursions(b, p, 0, stream, &linear))) return rc;
  hipLaunchKernelGGL(lat_ts_pass, dim3(64, b->N), dim3(kFbThreads), 0, stream, p, s, linear ? 1 : 0);
  p.out = like_S;
  if ((rc = fb_recursions(b, p, 0, stream, &linear))) return rc;
  if ((rc = fb_plain_posteriors(b, p, linear, stream))) return rc;
  hipLaunchKernelGGL(lat_ts_finish, dim3(64, b->N), dim3(256), 0, stream, p, s);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
