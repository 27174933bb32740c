// Complex Gaussian mixture model (cGMM) mask estimation for a ragged minibatch (include/pk2hip.h): per
// frequency bin an EM over the frames with one spatial covariance R_k and one weight alpha_k per class.  Lanes on bins
// everywhere, as in beamform.hip; no atomics, nothing read back.
//
//   factor      one thread per (utterance, class, bin), float64: R' = R + load I = L L^H, L^-1 rounded once to complex64 and
//               written [element][F], b = log alpha - 2 sum log L_jj.
//   E-pass      one wave per (utterance, 32 frames, 64 bins, class): z = L^-1 y as fmaf chains, q = sum |z_j|^2,
//               phi = max(q / C, 1e-10), l = b + log a - C log phi; l and phi go to the workspace.
//   softmax     one wave per (utterance, 32 frames, 64 bins): lambda over the classes with the maximum subtracted, the frame
//               terms of the log-likelihood summed in float64 per (part, bin).
//   M-step      the covariance pass of array_internal.h (cov_kernel, cov_reduce_kernel) with the weight lambda / phi and the
//               normaliser sum lambda (PosteriorWeights below): float32 chains in frame order per 32-frame part, the parts
//               added in part order in float64, the mirror the exact conjugate; the reduce kernel also writes log alpha.
#include <algorithm>

#include "array_internal.h"

namespace pk2 {

constexpr int kCgLanes = 64;                        // bins per workgroup (one wave)
constexpr int kCgPart = PK2_BF_FRAMES_PER_PART;     // frames per workgroup of every per-(t, f) pass
constexpr int kCgMaxK = PK2_BF_MAX_MASKS;

struct CgTab {
  const float2* spec[PK2_BF_MAX_UTTS];
  const float* act[PK2_BF_MAX_UTTS];                // (K, N), or null: every class active on every frame
  float* ell[PK2_BF_MAX_UTTS];                      // (K, N, F): what the E-pass writes and the softmax reads
  float* lam[PK2_BF_MAX_UTTS];                      // (K, N, F): what the softmax writes and the M-step reads (null: 1)
  float* phi[PK2_BF_MAX_UTTS];                      // (K, N, F) (null in the M-step: 1)
  Ragged rag;
};

// The weights of cov_kernel in the M-step: lambda_k / phi_k, the normaliser sum lambda_k; a null plane is 1.
template <int KA_>
struct PosteriorWeights {
  using Tab = CgTab;
  static constexpr int KA = KA_;
  const float* __restrict__ L;
  const float* __restrict__ P;
  __device__ __forceinline__ PosteriorWeights(const Tab& tab, int b) : L(tab.lam[b]), P(tab.phi[b]) {}
  __device__ __forceinline__ void load(int64_t o, int64_t NF, float (&m)[KA], float (&ms)[KA]) const {
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const float l = L ? L[k * NF + o] : 1.f;
      ms[k] += l;
      m[k] = P ? l / P[k * NF + o] : l;
    }
  }
};

// grid (utterances of the launch): the number of frames on which any class is active
__global__ void __launch_bounds__(256) cg_nact_kernel(const CgTab tab, int K, int32_t* __restrict__ nact) {
  __shared__ int s_n[256];
  const int b = blockIdx.x, tid = threadIdx.x, N = tab.rag.frames[b];
  const float* __restrict__ a = tab.act[b];
  int n = 0;
  if (a) {
    for (int t = tid; t < N; t += 256) {
      bool on = false;
      for (int k = 0; k < K; ++k) on = on || a[(int64_t)k * N + t] > 0.f;
      n += on ? 1 : 0;
    }
  }
  s_n[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_n[tid] += s_n[tid + o];
    __syncthreads();
  }
  if (tid == 0) nact[b] = a ? s_n[0] : N;
}

// grid (ceil(F / 64), utterances of the launch), K = 2: R_1 = (Re tr R_0 / C) I and alpha_k = 1 / 2
__global__ void __launch_bounds__(kCgLanes) cg_init_noise_kernel(int C, int F, float2* __restrict__ R,
                                                                 float* __restrict__ log_alpha) {
  const int f = blockIdx.x * kCgLanes + threadIdx.x, b = blockIdx.y;
  if (f >= F) return;
  const float2* __restrict__ R0 = R + (((int64_t)b * 2 + 0) * F + f) * C * C;
  float2* __restrict__ R1 = R + (((int64_t)b * 2 + 1) * F + f) * C * C;
  double tr = 0.0;
  for (int i = 0; i < C; ++i) tr += (double)R0[i * C + i].x;
  const float v = (float)(tr / C);
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) R1[i * C + j] = make_float2(i == j ? v : 0.f, 0.f);
  const float la = (float)log(0.5);
  log_alpha[((int64_t)b * 2 + 0) * F + f] = la;
  log_alpha[((int64_t)b * 2 + 1) * F + f] = la;
}

// grid (ceil(F / 64), utterances of the launch * K).  R (nb, K, F, C, C), log_alpha (nb, K, F) -> linv (nb, K, 2 pairs, F):
// the lower triangle of L^-1 row by row, (re, im); bias (nb, K, F); bad (nb, K, F): 1 where R is not finite or R' not positive
// definite (then L^-1 = I and b = 0); bad_acc: the same, or-ed over the iterations of one pk2_cgmm call.
__global__ void __launch_bounds__(kCgLanes) cg_factor_kernel(int C, int F, double diag_load, int first,
                                                             const float2* __restrict__ R, const float* __restrict__ log_alpha,
                                                             float* __restrict__ linv, float* __restrict__ bias,
                                                             int32_t* __restrict__ bad, int32_t* __restrict__ bad_acc) {
  const int f = blockIdx.x * kCgLanes + threadIdx.x;
  const int64_t bk = blockIdx.y;
  if (f >= F) return;
  constexpr int kC = PK2_BF_MAX_CHANNELS;
  const float2* __restrict__ src = R + (bk * F + f) * C * C;
  cd A[kC][kC], X[kC][kC];
  bool ok = true;
  double tr = 0.0;
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) {
      const float2 a = src[i * C + j];
      A[i][j] = cd{(double)a.x, (double)a.y};
      ok = ok && isfinite(a.x) && isfinite(a.y);
      if (i == j) tr += (double)a.x;
    }
  double logdet = 0.0;
  hermitian_cholesky(A, C, diag_load * tr / C + 1e-10, ok, &logdet);
  // X = L^-1, column by column: X[j][j] = 1 / L[j][j], X[i][j] = -(sum_{k = j}^{i - 1} L[i][k] X[k][j]) / L[i][i]
  if (ok) {
    for (int j = 0; j < C; ++j) {
      X[j][j] = cd{1.0 / A[j][j].x, 0.0};
      for (int i = j + 1; i < C; ++i) {
        cd s{0.0, 0.0};
        for (int k = j; k < i; ++k) {
          s.x += A[i][k].x * X[k][j].x - A[i][k].y * X[k][j].y;
          s.y += A[i][k].x * X[k][j].y + A[i][k].y * X[k][j].x;
        }
        const double inv = -1.0 / A[i][i].x;
        X[i][j] = cd{s.x * inv, s.y * inv};
        ok = ok && isfinite(X[i][j].x) && isfinite(X[i][j].y);
      }
      ok = ok && isfinite(X[j][j].x);
    }
    ok = ok && isfinite(logdet);
  }
  const int P2 = 2 * tri_pairs(C);
  float* __restrict__ dst = linv + bk * P2 * F + f;
  int p = 0;
  for (int i = 0; i < C; ++i)
    for (int j = 0; j <= i; ++j, ++p) {
      dst[(int64_t)(2 * p) * F] = ok ? (float)X[i][j].x : (i == j ? 1.f : 0.f);
      dst[(int64_t)(2 * p + 1) * F] = ok && i != j ? (float)X[i][j].y : 0.f;
    }
  bias[bk * F + f] = ok ? (float)((double)log_alpha[bk * F + f] - 2.0 * logdet) : 0.f;
  bad[bk * F + f] = ok ? 0 : 1;
  if (bad_acc) bad_acc[bk * F + f] = (first ? 0 : bad_acc[bk * F + f]) | (ok ? 0 : 1);
}

// grid (parts of the launch, ceil(F / 64), K): l_k and phi_k of one class for 32 frames of 64 bins
template <int C>
__global__ void __launch_bounds__(kCgLanes) cg_e_kernel(const CgTab tab, int B, int F, int K, const float* __restrict__ linv,
                                                        const float* __restrict__ bias) {
  const int part = blockIdx.x, k = blockIdx.z;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * kCgLanes + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kCgPart, t1 = min(t0 + kCgPart, N);
  const float2* __restrict__ Y = tab.spec[b];
  const float* __restrict__ A = tab.act[b];
  constexpr int P = tri_pairs(C);
  const int64_t bk = (int64_t)b * K + k;
  const float* __restrict__ src = linv + bk * 2 * P * F + f;
  float lr[P], li[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    lr[p] = src[(int64_t)(2 * p) * F];
    li[p] = src[(int64_t)(2 * p + 1) * F];
  }
  const float bk_f = bias[bk * F + f];
  const int64_t NF = (int64_t)N * F;
  float* __restrict__ ell = tab.ell[b] + k * NF;
  float* __restrict__ phi = tab.phi[b] + k * NF;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
    float2 y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = Y[c * NF + o];
    float q = 0.f;
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      float zr = 0.f, zi = 0.f;
#pragma unroll
      for (int j = 0; j <= i; ++j, ++p) {
        zr = fmaf(lr[p], y[j].x, zr);
        zi = fmaf(lr[p], y[j].y, zi);
        if (j != i) {
          zr = fmaf(-li[p], y[j].y, zr);
          zi = fmaf(li[p], y[j].x, zi);
        }
      }
      q = fmaf(zr, zr, q);
      q = fmaf(zi, zi, q);
    }
    const float ph = fmaxf(q / (float)C, 1e-10f);
    const float la = A ? logf(A[(int64_t)k * N + t]) : 0.f;      // log 0 = -inf: the class is off on this frame
    ell[o] = (bk_f + la) - (float)C * logf(ph);
    phi[o] = ph;
  }
}

// grid (parts of the launch, ceil(F / 64)).  bad: (nb, K, F) of the factorisation; ll_part: [part][F] float64.
__global__ void __launch_bounds__(kCgLanes) cg_softmax_kernel(const CgTab tab, int B, int F, int K, const int32_t* __restrict__ bad,
                                                              double* __restrict__ ll_part) {
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * kCgLanes + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kCgPart, t1 = min(t0 + kCgPart, N);
  const int64_t NF = (int64_t)N * F;
  const float* ell = tab.ell[b];      // lam may be the same plane: a frame's l_k are all read before its lambda_k are written
  float* lam = tab.lam[b];
  bool fail = false;
  for (int k = 0; k < K; ++k) fail = fail || bad[((int64_t)b * K + k) * F + f] != 0;
  const float uniform = 1.f / (float)K;
  double ll = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
    float l[kCgMaxK], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kCgMaxK; ++k) {
      l[k] = k < K ? ell[k * NF + o] : -INFINITY;
      mx = fmaxf(mx, l[k]);
    }
    if (fail) {
      for (int k = 0; k < K; ++k) lam[k * NF + o] = uniform;
    } else if (!(mx > -INFINITY)) {          // no active class on this frame
      for (int k = 0; k < K; ++k) lam[k * NF + o] = 0.f;
    } else {
      float e[kCgMaxK], s = 0.f;
#pragma unroll
      for (int k = 0; k < kCgMaxK; ++k) {
        e[k] = k < K ? expf(l[k] - mx) : 0.f;
        s += e[k];
      }
#pragma unroll
      for (int k = 0; k < kCgMaxK; ++k)
        if (k < K) lam[k * NF + o] = e[k] / s;
      ll += (double)(mx + logf(s));
    }
  }
  ll_part[(int64_t)part * F + f] = ll;
}

// grid (utterances of the launch): ll[b * stride] = sum over the parts and bins of ll_part, per bin in part order, the
// bins of a thread in order, the 256 threads in order
__global__ void __launch_bounds__(256) cg_ll_kernel(const CgTab tab, int F, const double* __restrict__ ll_part,
                                                    double* __restrict__ ll, int stride) {
  __shared__ double s_v[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  double v = 0.0;
  for (int f = tid; f < F; f += 256)
    for (int part = tab.rag.part_off[b]; part < tab.rag.part_off[b + 1]; ++part) v += ll_part[(int64_t)part * F + f];
  s_v[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += s_v[i];
    ll[(int64_t)b * stride] = s;
  }
}

// grid (ceil(F / 64), utterances of the launch), K = 2: class 0 becomes the class with the larger
// ||R||_F^2 / (Re tr R)^2; a swap exchanges the masks, R and log alpha of the bin
__global__ void __launch_bounds__(kCgLanes) cg_order_kernel(const CgTab tab, int C, int F, float2* __restrict__ R,
                                                            float* __restrict__ log_alpha) {
  const int f = blockIdx.x * kCgLanes + threadIdx.x, b = blockIdx.y;
  if (f >= F) return;
  float2* __restrict__ R0 = R + (((int64_t)b * 2 + 0) * F + f) * C * C;
  float2* __restrict__ R1 = R + (((int64_t)b * 2 + 1) * F + f) * C * C;
  double pur[2];
  for (int k = 0; k < 2; ++k) {
    const float2* __restrict__ M = k ? R1 : R0;
    double fro = 0.0, tr = 0.0;
    for (int i = 0; i < C; ++i)
      for (int j = 0; j < C; ++j) {
        const float2 a = M[i * C + j];
        fro += (double)a.x * (double)a.x + (double)a.y * (double)a.y;
        if (i == j) tr += (double)a.x;
      }
    pur[k] = fro / (tr * tr);
  }
  if (!(pur[1] > pur[0])) return;
  for (int e = 0; e < C * C; ++e) {
    const float2 a = R0[e];
    R0[e] = R1[e];
    R1[e] = a;
  }
  float* __restrict__ a0 = log_alpha + ((int64_t)b * 2 + 0) * F + f;
  float* __restrict__ a1 = log_alpha + ((int64_t)b * 2 + 1) * F + f;
  const float a = *a0;
  *a0 = *a1;
  *a1 = a;
  const int N = tab.rag.frames[b];
  float* __restrict__ lam = tab.lam[b];
  const int64_t NF = (int64_t)N * F;
  for (int t = 0; t < N; ++t) {
    const int64_t o = (int64_t)t * F + f;
    const float m = lam[o];
    lam[o] = lam[NF + o];
    lam[NF + o] = m;
  }
}

static int cg_check_shape(const char* who, int32_t B, int32_t C, int32_t F, int32_t K) {
  if (int rc = check_shape(who, B, C, F)) return rc;
  PK2_REQUIRE(K >= 2 && K <= PK2_BF_MAX_MASKS, "%s: %d classes (2 to %d)", who, K, PK2_BF_MAX_MASKS);
  return PK2_OK;
}

// The workspace of one call: the per-(k, t, f) planes of all utterances, then what a launch of PK2_BF_MAX_UTTS needs.
struct CgWork {
  float *ell, *phi, *cov_part, *linv, *bias;
  double* ll_part;
  int32_t *bad, *bad_acc, *nact;
  size_t bytes;
};

static CgWork cg_carve(void* base, const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K) {
  int64_t total = 0, parts = 0;
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    int64_t p = 0;
    for (int b = b0; b < std::min<int>(B, b0 + PK2_BF_MAX_UTTS); ++b) {
      total += frames[b];
      p += (frames[b] + kCgPart - 1) / kCgPart;
    }
    parts = std::max(parts, p);
  }
  Carver cv(base);
  CgWork w;
  w.ell = cv.take<float>((size_t)total * K * F);
  w.phi = cv.take<float>((size_t)total * K * F);
  w.cov_part = cv.take<float>((size_t)parts * K * cov_entries(C) * F);
  w.ll_part = cv.take<double>((size_t)parts * F);
  w.linv = cv.take<float>((size_t)B * K * 2 * tri_pairs(C) * F);
  w.bias = cv.take<float>((size_t)B * K * F);
  w.bad = cv.take<int32_t>((size_t)B * K * F);
  w.bad_acc = cv.take<int32_t>((size_t)B * K * F);
  w.nact = cv.take<int32_t>((size_t)B);
  w.bytes = cv.bytes();
  return w;
}

// the table of utterances [b0, b0 + nb) with its spectra and header; *parts: the parts of the launch
static int cg_fill(const char* who, CgTab& tab, const float* const* spec, const int32_t* frames, int b0, int nb, int64_t* parts) {
  memset(&tab, 0, sizeof(tab));
  for (int b = 0; b < nb; ++b) tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
  return fill_ragged(who, tab.rag, frames, b0, nb, kCgPart, parts);
}

static unsigned cg_tiles(int F) { return (unsigned)((F + kCgLanes - 1) / kCgLanes); }

// The M-step of one launch: tab.lam / tab.phi -> R and log_alpha of the nb utterances (pointers already at b0)
static void cg_mstep(const CgTab& tab, int nb, int64_t parts, int C, int F, int K, float* cov_part, const int32_t* nact,
                     float2* R, float* log_alpha, hipStream_t stream) {
  dispatch_channels(C, [&](auto c) {
    constexpr int Cc = decltype(c)::value;
    if (K == 2) cov_launch<Cc, PosteriorWeights<2>>(tab, nb, parts, F, cov_part, R, nact, log_alpha, stream);
    else if (K == 3) cov_launch<Cc, PosteriorWeights<3>>(tab, nb, parts, F, cov_part, R, nact, log_alpha, stream);
    else cov_launch<Cc, PosteriorWeights<4>>(tab, nb, parts, F, cov_part, R, nact, log_alpha, stream);
  });
}

// The E-step of one launch: linv / bias / bad (at b0) and the spectra -> tab.ell, tab.phi, tab.lam, ll[b * stride]
static void cg_estep(const CgTab& tab, int nb, int64_t parts, int C, int F, int K, const float* linv, const float* bias,
                     const int32_t* bad, double* ll_part, double* ll, int stride, hipStream_t stream) {
  const dim3 egrid((unsigned)parts, cg_tiles(F), (unsigned)K);
  dispatch_channels(C, [&](auto c) {
    hipLaunchKernelGGL(cg_e_kernel<decltype(c)::value>, egrid, dim3(kCgLanes), 0, stream, tab, nb, F, K, linv, bias);
  });
  hipLaunchKernelGGL(cg_softmax_kernel, dim3((unsigned)parts, cg_tiles(F)), dim3(kCgLanes), 0, stream, tab, nb, F, K, bad,
                     ll_part);
  hipLaunchKernelGGL(cg_ll_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, F, ll_part, ll, stride);
}

}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_cgmm_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K) {
  if (!frames || B < 1 || C < 1 || C > PK2_BF_MAX_CHANNELS || F < 1 || F > 4097 || K < 2 || K > PK2_BF_MAX_MASKS) return 0;
  for (int b = 0; b < B; ++b)
    if (frames[b] < 1 || frames[b] > (1 << 24)) return 0;
  return cg_carve(nullptr, frames, B, C, F, K).bytes;
}

extern "C" int pk2_cgmm_init(const float* const* spec, const float* const* init, const float* const* activity,
                             const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K, void* work, size_t work_bytes,
                             float* R, float* log_alpha, void* stream_) {
  if (int rc = cg_check_shape("cgmm_init", B, C, F, K)) return rc;
  PK2_REQUIRE(init || K == 2, "cgmm_init: %d classes need initial masks (without them K = 2)", K);
  PK2_REQUIRE(work && R && log_alpha, "cgmm_init: null pointer");
  if (int rc = check_frames("cgmm_init", frames, B)) return rc;
  if (int rc = check_table("cgmm_init", "the spectrum", spec, B)) return rc;
  if (init)
    if (int rc = check_table("cgmm_init", "the initial masks", init, B)) return rc;
  if (activity)
    if (int rc = check_table("cgmm_init", "the activity", activity, B)) return rc;
  const CgWork w = cg_carve(work, frames, B, C, F, K);
  PK2_REQUIRE(work_bytes >= w.bytes, "cgmm_init: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    CgTab tab;
    int64_t parts;
    if (int rc = cg_fill("cgmm_init", tab, spec, frames, b0, nb, &parts)) return rc;
    for (int b = 0; b < nb; ++b) {
      tab.lam[b] = init ? const_cast<float*>(init[b0 + b]) : nullptr;
      tab.act[b] = activity ? activity[b0 + b] : nullptr;
    }
    float2* Rb = reinterpret_cast<float2*>(R) + (int64_t)b0 * K * F * C * C;
    float* lab = log_alpha + (int64_t)b0 * K * F;
    hipLaunchKernelGGL(cg_nact_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, K, w.nact + b0);
    PK2_LAUNCH_CHECK();
    cg_mstep(tab, nb, parts, C, F, K, w.cov_part, w.nact + b0, Rb, lab, stream);
    PK2_LAUNCH_CHECK();
    if (!init) {
      hipLaunchKernelGGL(cg_init_noise_kernel, dim3(cg_tiles(F), (unsigned)nb), dim3(kCgLanes), 0, stream, C, F, Rb, lab);
      PK2_LAUNCH_CHECK();
    }
  }
  return PK2_OK;
}

extern "C" int pk2_cgmm_factor(const float* R, const float* log_alpha, int32_t B, int32_t C, int32_t F, int32_t K,
                               double diag_load, float* linv, float* bias, int32_t* bad, int32_t* nonfinite, void* stream_) {
  if (int rc = cg_check_shape("cgmm_factor", B, C, F, K)) return rc;
  PK2_REQUIRE(B <= 8192, "cgmm_factor: %d utterances in one call (at most 8192)", B);
  PK2_REQUIRE(diag_load >= 0.0 && diag_load < 1e30, "cgmm_factor: diag_load %g must be finite and >= 0", diag_load);
  PK2_REQUIRE(R && log_alpha && linv && bias && bad && nonfinite, "cgmm_factor: null pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(cg_factor_kernel, dim3(cg_tiles(F), (unsigned)(B * K)), dim3(kCgLanes), 0, stream, C, F, diag_load, 1,
                     reinterpret_cast<const float2*>(R), log_alpha, linv, bias, bad, (int32_t*)nullptr);
  PK2_LAUNCH_CHECK();
  hipLaunchKernelGGL(any_flag_kernel<256>, dim3((unsigned)B), dim3(256), 0, stream, bad, K * F, nonfinite);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_cgmm_posteriors(const float* const* spec, const float* const* activity, const int32_t* frames, int32_t B,
                                   int32_t C, int32_t F, int32_t K, const float* linv, const float* bias, const int32_t* bad,
                                   void* work, size_t work_bytes, float* const* lam, float* const* phi, double* ll,
                                   void* stream_) {
  if (int rc = cg_check_shape("cgmm_posteriors", B, C, F, K)) return rc;
  PK2_REQUIRE(linv && bias && bad && work && ll, "cgmm_posteriors: null pointer");
  if (int rc = check_frames("cgmm_posteriors", frames, B)) return rc;
  if (int rc = check_table("cgmm_posteriors", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("cgmm_posteriors", "lam", lam, B)) return rc;
  if (int rc = check_table("cgmm_posteriors", "phi", phi, B)) return rc;
  if (activity)
    if (int rc = check_table("cgmm_posteriors", "the activity", activity, B)) return rc;
  const CgWork w = cg_carve(work, frames, B, C, F, K);
  PK2_REQUIRE(work_bytes >= w.bytes, "cgmm_posteriors: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    CgTab tab;
    int64_t parts;
    if (int rc = cg_fill("cgmm_posteriors", tab, spec, frames, b0, nb, &parts)) return rc;
    for (int b = 0; b < nb; ++b) {
      tab.act[b] = activity ? activity[b0 + b] : nullptr;
      tab.ell[b] = tab.lam[b] = lam[b0 + b];      // l_k is replaced by lambda_k in place
      tab.phi[b] = phi[b0 + b];
    }
    const int64_t kf = (int64_t)b0 * K * F;
    cg_estep(tab, nb, parts, C, F, K, linv + kf * 2 * tri_pairs(C), bias + kf, bad + kf, w.ll_part, ll + b0, 1, stream);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}

extern "C" int pk2_cgmm_update(const float* const* spec, const float* const* lam, const float* const* phi,
                               const float* const* activity, const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K,
                               void* work, size_t work_bytes, float* R, float* log_alpha, void* stream_) {
  if (int rc = cg_check_shape("cgmm_update", B, C, F, K)) return rc;
  PK2_REQUIRE(work && R && log_alpha, "cgmm_update: null pointer");
  if (int rc = check_frames("cgmm_update", frames, B)) return rc;
  if (int rc = check_table("cgmm_update", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("cgmm_update", "lam", lam, B)) return rc;
  if (int rc = check_table("cgmm_update", "phi", phi, B)) return rc;
  if (activity)
    if (int rc = check_table("cgmm_update", "the activity", activity, B)) return rc;
  const CgWork w = cg_carve(work, frames, B, C, F, K);
  PK2_REQUIRE(work_bytes >= w.bytes, "cgmm_update: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    CgTab tab;
    int64_t parts;
    if (int rc = cg_fill("cgmm_update", tab, spec, frames, b0, nb, &parts)) return rc;
    for (int b = 0; b < nb; ++b) {
      tab.act[b] = activity ? activity[b0 + b] : nullptr;
      tab.lam[b] = const_cast<float*>(lam[b0 + b]);
      tab.phi[b] = const_cast<float*>(phi[b0 + b]);
    }
    hipLaunchKernelGGL(cg_nact_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, K, w.nact + b0);
    PK2_LAUNCH_CHECK();
    cg_mstep(tab, nb, parts, C, F, K, w.cov_part, w.nact + b0, reinterpret_cast<float2*>(R) + (int64_t)b0 * K * F * C * C,
             log_alpha + (int64_t)b0 * K * F, stream);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}

extern "C" int pk2_cgmm(const float* const* spec, const float* const* init, const float* const* activity, const int32_t* frames,
                        int32_t B, int32_t C, int32_t F, int32_t K, int32_t iters, double diag_load, int32_t purity, void* work,
                        size_t work_bytes, float* const* masks, float* R, float* log_alpha, double* ll, int32_t* nonfinite,
                        void* stream_) {
  if (int rc = cg_check_shape("cgmm", B, C, F, K)) return rc;
  PK2_REQUIRE(iters >= 1 && iters <= PK2_CGMM_MAX_ITERS, "cgmm: %d iterations (1 to %d)", iters, PK2_CGMM_MAX_ITERS);
  PK2_REQUIRE(diag_load >= 0.0 && diag_load < 1e30, "cgmm: diag_load %g must be finite and >= 0", diag_load);
  PK2_REQUIRE(init || K == 2, "cgmm: %d classes need initial masks (without them K = 2)", K);
  PK2_REQUIRE(!purity || K == 2, "cgmm: the purity order is defined for two classes, not %d", K);
  PK2_REQUIRE(work && R && log_alpha && ll && nonfinite, "cgmm: null pointer");
  if (int rc = check_frames("cgmm", frames, B)) return rc;
  if (int rc = check_table("cgmm", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("cgmm", "the masks", masks, B)) return rc;
  if (init)
    if (int rc = check_table("cgmm", "the initial masks", init, B)) return rc;
  if (activity)
    if (int rc = check_table("cgmm", "the activity", activity, B)) return rc;
  const CgWork w = cg_carve(work, frames, B, C, F, K);
  PK2_REQUIRE(work_bytes >= w.bytes, "cgmm: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int64_t frame_off = 0;
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    CgTab tab;
    int64_t parts;
    if (int rc = cg_fill("cgmm", tab, spec, frames, b0, nb, &parts)) return rc;
    const int64_t kf = (int64_t)b0 * K * F;
    float2* Rb = reinterpret_cast<float2*>(R) + kf * C * C;
    float* lab = log_alpha + kf;
    float* linv = w.linv + kf * 2 * tri_pairs(C);
    for (int b = 0; b < nb; ++b) {
      tab.act[b] = activity ? activity[b0 + b] : nullptr;
      tab.lam[b] = init ? const_cast<float*>(init[b0 + b]) : nullptr;
    }
    hipLaunchKernelGGL(cg_nact_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, K, w.nact + b0);
    PK2_LAUNCH_CHECK();
    cg_mstep(tab, nb, parts, C, F, K, w.cov_part, w.nact + b0, Rb, lab, stream);
    PK2_LAUNCH_CHECK();
    if (!init) {
      hipLaunchKernelGGL(cg_init_noise_kernel, dim3(cg_tiles(F), (unsigned)nb), dim3(kCgLanes), 0, stream, C, F, Rb, lab);
      PK2_LAUNCH_CHECK();
    }
    for (int b = 0; b < nb; ++b) {
      tab.ell[b] = w.ell + frame_off * K * F;
      tab.phi[b] = w.phi + frame_off * K * F;
      tab.lam[b] = tab.ell[b];
      frame_off += frames[b0 + b];
    }
    for (int it = 0; it < iters; ++it) {
      hipLaunchKernelGGL(cg_factor_kernel, dim3(cg_tiles(F), (unsigned)(nb * K)), dim3(kCgLanes), 0, stream, C, F, diag_load,
                         it == 0 ? 1 : 0, Rb, lab, linv, w.bias + kf, w.bad + kf, w.bad_acc + kf);
      PK2_LAUNCH_CHECK();
      if (it == iters - 1)
        for (int b = 0; b < nb; ++b) tab.lam[b] = masks[b0 + b];      // only the last posteriors leave the workspace
      cg_estep(tab, nb, parts, C, F, K, linv, w.bias + kf, w.bad + kf, w.ll_part, ll + (int64_t)b0 * iters + it, iters, stream);
      PK2_LAUNCH_CHECK();
      cg_mstep(tab, nb, parts, C, F, K, w.cov_part, w.nact + b0, Rb, lab, stream);
      PK2_LAUNCH_CHECK();
    }
    if (purity) {
      hipLaunchKernelGGL(cg_order_kernel, dim3(cg_tiles(F), (unsigned)nb), dim3(kCgLanes), 0, stream, tab, C, F, Rb, lab);
      PK2_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(any_flag_kernel<256>, dim3((unsigned)nb), dim3(256), 0, stream, w.bad_acc + kf, K * F, nonfinite + b0);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}
