// Mask-based MVDR beamforming for a ragged minibatch (include/pk2hip.h): masked spatial covariances, Souden's
// MVDR weights, and the weighted sum over the channels.
//
//   pk2_bf_cov           the covariance pass of array_internal.h (cov_kernel, cov_reduce_kernel) weighted with the masks:
//                        MaskWeights below.  C and the number of masks are template parameters.
//   pk2_bf_mvdr_weights  one thread per (utterance, bin): float32 in, float64 arithmetic (loading, Cholesky, C solves, trace),
//                        complex64 out.  For the 'snr' reference it leaves every candidate's weights and SNR terms in the
//                        workspace; one workgroup per utterance then adds the terms over f in bin order, picks the channel
//                        and copies its weights.  Nothing returns to the host.
//   pk2_bf_apply         lanes on bins, the C weights of a bin in registers, one pass over the spectrum.
#include <algorithm>

#include "array_internal.h"

namespace pk2 {

constexpr int kBfLanes = 64;                        // bins per workgroup (one wave)
constexpr int kBfApplyFrames = 32;                  // frames per workgroup of the apply pass

struct BfCovTab {
  const float2* spec[PK2_BF_MAX_UTTS];
  const float* mask[PK2_BF_MAX_UTTS * PK2_BF_MAX_MASKS];
  Ragged rag;
};
struct BfApplyTab {
  const float2* spec[PK2_BF_MAX_UTTS];
  const float2* w[PK2_BF_MAX_UTTS];
  float2* out[PK2_BF_MAX_UTTS];
  Ragged rag;
};
struct BfPhiTab {
  const float2* phi_s[PK2_BF_MAX_UTTS];
  const float2* phi_n[PK2_BF_MAX_UTTS];
};

// The weights of cov_kernel: KA_ masks, each its own normaliser; COMP: KA_ == 2 from one mask m: (m, 1 - m).
template <int KA_, bool COMP>
struct MaskWeights {
  using Tab = BfCovTab;
  static constexpr int KA = KA_, KM = COMP ? 1 : KA_;
  const float* __restrict__ M[KM];
  __device__ __forceinline__ MaskWeights(const Tab& tab, int b) {
#pragma unroll
    for (int k = 0; k < KM; ++k) M[k] = tab.mask[b * PK2_BF_MAX_MASKS + k];
  }
  __device__ __forceinline__ void load(int64_t o, int64_t, float (&m)[KA], float (&ms)[KA]) const {
#pragma unroll
    for (int k = 0; k < KM; ++k) m[k] = M[k][o];
    if (COMP) m[KA - 1] = 1.f - m[0];
#pragma unroll
    for (int k = 0; k < KA; ++k) ms[k] += m[k];
  }
};

// One thread per (utterance, bin).  ref >= 0: w (B, F, C) gets the weights of that channel.  ref < 0 ('snr'): cand
// (B, C, F, C) gets every candidate's weights and terms (B, C, 2, F) the numerator and denominator of its SNR at this bin.
// bad (B, F): 1 where the bin fell back to e_r on non-finite input.
__global__ void __launch_bounds__(kBfLanes) bf_weights_kernel(const BfPhiTab tab, int C, int F, int ref, double diag_load,
                                                              float2* __restrict__ w, float2* __restrict__ cand,
                                                              double* __restrict__ terms, int32_t* __restrict__ bad) {
  const int f = blockIdx.x * kBfLanes + threadIdx.x, b = blockIdx.y;
  if (f >= F) return;
  constexpr int kC = PK2_BF_MAX_CHANNELS;
  const float2* __restrict__ Ps = tab.phi_s[b] + (int64_t)f * C * C;
  const float2* __restrict__ Pn = tab.phi_n[b] + (int64_t)f * C * C;
  cd A[kC][kC], G[kC][kC];
  bool ok = true;
  double tr = 0.0;
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) {
      const float2 a = Pn[i * C + j], s = Ps[i * C + j];
      A[i][j] = cd{(double)a.x, (double)a.y};
      G[i][j] = cd{(double)s.x, (double)s.y};
      ok = ok && isfinite(a.x) && isfinite(a.y) && isfinite(s.x) && isfinite(s.y);
      if (i == j) tr += (double)a.x;
    }
  const double load = diag_load * tr / C + 1e-10;
  hermitian_cholesky(A, C, load, ok);
  cd trg{0.0, 0.0};
  if (ok) {
    // G = A^-1 Phi_s column by column: L y = s, then L^H g = y
    for (int c = 0; c < C; ++c) {
      for (int i = 0; i < C; ++i) {
        cd s = G[i][c];
        for (int k = 0; k < i; ++k) { const cd q = cmul(A[i][k], G[k][c]); s.x -= q.x; s.y -= q.y; }
        const double inv = 1.0 / A[i][i].x;
        G[i][c] = cd{s.x * inv, s.y * inv};
      }
      for (int i = C - 1; i >= 0; --i) {
        cd s = G[i][c];
        for (int k = i + 1; k < C; ++k) {      // conj(L[k][i]) g[k]
          const cd l = A[k][i];
          const cd g = G[k][c];
          s.x -= l.x * g.x + l.y * g.y;
          s.y -= l.x * g.y - l.y * g.x;
        }
        const double inv = 1.0 / A[i][i].x;
        G[i][c] = cd{s.x * inv, s.y * inv};
      }
    }
    for (int c = 0; c < C; ++c) { trg.x += G[c][c].x; trg.y += G[c][c].y; }
    ok = isfinite(trg.x) && isfinite(trg.y);
  }
  const bool pass = !ok || !(trg.x * trg.x + trg.y * trg.y > 1e-40);      // |tr G| <= 1e-20: the reference channel passes
  bad[(int64_t)b * F + f] = ok ? 0 : 1;
  const int c0 = ref >= 0 ? ref : 0, c1 = ref >= 0 ? ref + 1 : C;
  for (int r = c0; r < c1; ++r) {
    cd wv[kC];
    bool unit = pass;
    if (!unit) {
      for (int i = 0; i < C; ++i) {
        wv[i] = cdivc(G[i][r], trg);
        unit = unit || !isfinite(wv[i].x) || !isfinite(wv[i].y);
      }
    }
    if (unit)
      for (int i = 0; i < C; ++i) wv[i] = cd{i == r ? 1.0 : 0.0, 0.0};
    float2* __restrict__ dst = ref >= 0 ? w + ((int64_t)b * F + f) * C : cand + (((int64_t)b * C + r) * F + f) * C;
    for (int i = 0; i < C; ++i) dst[i] = make_float2((float)wv[i].x, (float)wv[i].y);
    if (ref < 0) {
      // Re(w^H Phi_s w) and Re(w^H Phi_n' w) from the float32 inputs (A and G were overwritten); 0 on a non-finite bin
      double num = 0.0, den = 0.0;
      if (ok) {
        for (int i = 0; i < C; ++i)
          for (int j = 0; j < C; ++j) {
            const cd q = cmulc(wv[j], wv[i]);      // w_j conj(w_i)
            const float2 s = Ps[i * C + j], a = Pn[i * C + j];
            num += (double)s.x * q.x - (double)s.y * q.y;
            den += (double)a.x * q.x - (double)a.y * q.y;
            if (i == j) den += load * q.x;
          }
      }
      terms[(((int64_t)b * C + r) * 2 + 0) * F + f] = num;
      terms[(((int64_t)b * C + r) * 2 + 1) * F + f] = den;
    }
  }
}

// One workgroup per utterance: the non-finite flag, and for 'snr' the sums over f in bin order, the choice and the copy.
__global__ void __launch_bounds__(256) bf_select_kernel(int C, int F, int ref, const float2* __restrict__ cand,
                                                        const double* __restrict__ terms, const int32_t* __restrict__ bad,
                                                        float2* __restrict__ w, int32_t* __restrict__ ref_index,
                                                        int32_t* __restrict__ nonfinite) {
  __shared__ double s_snr[PK2_BF_MAX_CHANNELS];
  __shared__ int s_any[256];
  __shared__ int s_ref;
  const int b = blockIdx.x, tid = threadIdx.x;
  int any = 0;
  for (int f = tid; f < F; f += 256) any |= bad[(int64_t)b * F + f];
  s_any[tid] = any;
  if (ref < 0 && tid < C) {
    const double* __restrict__ num = terms + (((int64_t)b * C + tid) * 2 + 0) * F;
    const double* __restrict__ den = num + F;
    double sn = 0.0, sd = 0.0;
    for (int f = 0; f < F; ++f) { sn += num[f]; sd += den[f]; }
    s_snr[tid] = sn / sd;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int i = 0; i < 256; ++i) a |= s_any[i];
    nonfinite[b] = a;
    int r = ref >= 0 ? ref : 0;
    if (ref < 0)
      for (int c = 1; c < C; ++c)
        if (s_snr[c] > s_snr[r]) r = c;        // ties (and NaN) keep the lower index
    s_ref = r;
    ref_index[b] = r;
  }
  if (ref >= 0) return;
  __syncthreads();
  const int r = s_ref;
  const float2* __restrict__ src = cand + ((int64_t)b * C + r) * F * C;
  float2* __restrict__ dst = w + (int64_t)b * F * C;
  for (int i = tid; i < F * C; i += 256) dst[i] = src[i];
}

// grid (parts of the launch, ceil(F / 64)): X[t, f] = sum_c conj(w[f, c]) Y[c, t, f], c ascending
template <int C>
__global__ void __launch_bounds__(kBfLanes) bf_apply_kernel(const BfApplyTab tab, int B, int F) {
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * kBfLanes + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kBfApplyFrames, t1 = min(t0 + kBfApplyFrames, N);
  const float2* __restrict__ Y = tab.spec[b];
  float2* __restrict__ X = tab.out[b];
  float2 wv[C];
#pragma unroll
  for (int c = 0; c < C; ++c) wv[c] = tab.w[b][(int64_t)f * C + c];
  const int64_t NF = (int64_t)N * F;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
    float xr = 0.f, xi = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float2 y = Y[c * NF + o];
      xr = fmaf(wv[c].x, y.x, xr); xr = fmaf(wv[c].y, y.y, xr);
      xi = fmaf(wv[c].x, y.y, xi); xi = fmaf(-wv[c].y, y.x, xi);
    }
    X[o] = make_float2(xr, xi);
  }
}

template <int C>
static void bf_cov_launch(int KA, bool comp, const BfCovTab& tab, int nb, int64_t parts, int F, float* work, float2* phi,
                          hipStream_t stream) {
  if (comp) cov_launch<C, MaskWeights<2, true>>(tab, nb, parts, F, work, phi, nullptr, nullptr, stream);
  else if (KA == 1) cov_launch<C, MaskWeights<1, false>>(tab, nb, parts, F, work, phi, nullptr, nullptr, stream);
  else if (KA == 2) cov_launch<C, MaskWeights<2, false>>(tab, nb, parts, F, work, phi, nullptr, nullptr, stream);
  else if (KA == 3) cov_launch<C, MaskWeights<3, false>>(tab, nb, parts, F, work, phi, nullptr, nullptr, stream);
  else cov_launch<C, MaskWeights<4, false>>(tab, nb, parts, F, work, phi, nullptr, nullptr, stream);
}

static size_t bf_cov_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t KA) {
  int64_t parts = 0;
  for (int b = 0; b < B; ++b) parts += (frames[b] + kCovPart - 1) / kCovPart;
  return align_up((size_t)parts * KA * cov_entries(C) * F * sizeof(float), 256);
}

static size_t bf_weights_bytes(int32_t B, int32_t C, int32_t F) {
  Carver cv(nullptr);
  cv.take<int32_t>((size_t)B * F);
  cv.take<double>((size_t)B * C * 2 * F);
  cv.take<float2>((size_t)B * C * F * C);
  return cv.bytes();
}

}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_bf_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K, int32_t complement) {
  if (B < 1 || C < 1 || C > PK2_BF_MAX_CHANNELS || F < 1 || F > 4097) return 0;
  size_t need = bf_weights_bytes(B, C, F);
  if (frames) {
    if (K < 1 || K > PK2_BF_MAX_MASKS || (complement && K != 1)) return 0;
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > (1 << 24)) return 0;
    need = std::max(need, bf_cov_bytes(frames, B, C, F, complement ? 2 : K));
  }
  return need;
}

extern "C" int pk2_bf_cov(const float* const* spec, const float* const* masks, const int32_t* frames, int32_t B, int32_t C,
                          int32_t F, int32_t K, int32_t complement, void* work, size_t work_bytes, float* phi, void* stream_) {
  if (int rc = check_shape("bf_cov", B, C, F)) return rc;
  PK2_REQUIRE(K >= 1 && K <= PK2_BF_MAX_MASKS, "bf_cov: %d masks (1 to %d)", K, PK2_BF_MAX_MASKS);
  PK2_REQUIRE(!complement || K == 1, "bf_cov: complement needs exactly one mask, got %d", K);
  PK2_REQUIRE(spec && masks && work && phi, "bf_cov: null pointer");
  if (int rc = check_frames("bf_cov", frames, B)) return rc;
  for (int b = 0; b < B; ++b) {
    PK2_REQUIRE(spec[b], "bf_cov: spectrum %d is null", b);
    for (int k = 0; k < K; ++k) PK2_REQUIRE(masks[b * K + k], "bf_cov: mask %d of utterance %d is null", k, b);
  }
  const int KA = complement ? 2 : K;
  PK2_REQUIRE(work_bytes >= bf_cov_bytes(frames, B, C, F, KA), "bf_cov: workspace of %zu bytes, %zu needed", work_bytes,
              bf_cov_bytes(frames, B, C, F, KA));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* wk = static_cast<float*>(work);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    BfCovTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      for (int k = 0; k < K; ++k) tab.mask[b * PK2_BF_MAX_MASKS + k] = masks[(b0 + b) * K + k];
    }
    int64_t parts;
    if (int rc = fill_ragged("bf_cov", tab.rag, frames, b0, nb, kCovPart, &parts)) return rc;
    float2* out = reinterpret_cast<float2*>(phi) + (int64_t)b0 * KA * F * C * C;
    dispatch_channels(C, [&](auto c) { bf_cov_launch<decltype(c)::value>(KA, complement != 0, tab, nb, parts, F, wk, out, stream); });
    PK2_LAUNCH_CHECK();
    wk += parts * KA * cov_entries(C) * F;
  }
  return PK2_OK;
}

extern "C" int pk2_bf_mvdr_weights(const float* const* phi_s, const float* const* phi_n, int32_t B, int32_t C, int32_t F,
                                   int32_t ref, double diag_load, void* work, size_t work_bytes, float* w, int32_t* ref_index,
                                   int32_t* nonfinite, void* stream_) {
  if (int rc = check_shape("bf_mvdr_weights", B, C, F)) return rc;
  PK2_REQUIRE(ref == PK2_BF_REF_SNR || (ref >= 0 && ref < C), "bf_mvdr_weights: ref %d outside [0, %d) and not PK2_BF_REF_SNR",
              ref, C);
  PK2_REQUIRE(diag_load >= 0.0 && diag_load < 1e30, "bf_mvdr_weights: diag_load %g must be finite and >= 0", diag_load);
  PK2_REQUIRE(phi_s && phi_n && work && w && ref_index && nonfinite, "bf_mvdr_weights: null pointer");
  for (int b = 0; b < B; ++b) PK2_REQUIRE(phi_s[b] && phi_n[b], "bf_mvdr_weights: covariance %d is null", b);
  PK2_REQUIRE(work_bytes >= bf_weights_bytes(B, C, F), "bf_mvdr_weights: workspace of %zu bytes, %zu needed", work_bytes,
              bf_weights_bytes(B, C, F));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Carver cv(work);
  int32_t* bad = cv.take<int32_t>((size_t)B * F);
  double* terms = cv.take<double>((size_t)B * C * 2 * F);
  float2* cand = cv.take<float2>((size_t)B * C * F * C);
  float2* w2 = reinterpret_cast<float2*>(w);
  const unsigned tiles = (unsigned)((F + kBfLanes - 1) / kBfLanes);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    BfPhiTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.phi_s[b] = reinterpret_cast<const float2*>(phi_s[b0 + b]);
      tab.phi_n[b] = reinterpret_cast<const float2*>(phi_n[b0 + b]);
    }
    hipLaunchKernelGGL(bf_weights_kernel, dim3(tiles, (unsigned)nb), dim3(kBfLanes), 0, stream, tab, C, F, ref, diag_load,
                       w2 + (int64_t)b0 * F * C, cand + (int64_t)b0 * C * F * C, terms + (int64_t)b0 * C * 2 * F,
                       bad + (int64_t)b0 * F);
    PK2_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bf_select_kernel, dim3((unsigned)B), dim3(256), 0, stream, C, F, ref, cand, terms, bad, w2, ref_index,
                     nonfinite);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_bf_apply(const float* const* spec, const float* const* w, const int32_t* frames, int32_t B, int32_t C,
                            int32_t F, float* const* out, void* stream_) {
  if (int rc = check_shape("bf_apply", B, C, F)) return rc;
  PK2_REQUIRE(spec && w && out, "bf_apply: null pointer");
  if (int rc = check_frames("bf_apply", frames, B)) return rc;
  for (int b = 0; b < B; ++b) PK2_REQUIRE(spec[b] && w[b] && out[b], "bf_apply: a pointer of utterance %d is null", b);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned tiles = (unsigned)((F + kBfLanes - 1) / kBfLanes);
  for (int b0 = 0; b0 < B; b0 += PK2_BF_MAX_UTTS) {
    const int nb = std::min<int>(PK2_BF_MAX_UTTS, B - b0);
    BfApplyTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      tab.w[b] = reinterpret_cast<const float2*>(w[b0 + b]);
      tab.out[b] = reinterpret_cast<float2*>(out[b0 + b]);
    }
    int64_t parts;
    if (int rc = fill_ragged("bf_apply", tab.rag, frames, b0, nb, kBfApplyFrames, &parts)) return rc;
    const dim3 grid((unsigned)parts, tiles), block(kBfLanes);
    dispatch_channels(C, [&](auto c) {
      hipLaunchKernelGGL(bf_apply_kernel<decltype(c)::value>, grid, block, 0, stream, tab, nb, F);
    });
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}
