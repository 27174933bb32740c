// Frequency permutation alignment of cGMM masks for a ragged minibatch (include/pk2hip.h): a blind EM runs
// per bin, so class k of one bin and class k of the next are unrelated; the bins are matched by how their posteriors move
// over time (Sawada et al. 2011).  Per utterance pi_f, a permutation of the K classes per bin, out[a, t, f] = lam[pi_f[a], t, f].
// A permutation travels as one 32-bit word, byte a = pi[a].  No atomics, no workgroup waits on another, nothing read back.
//
//   features    one workgroup per (utterance, class, 64 bins): mean and norm over the frames in float64 (lanes on bins, the
//               sixteen waves on frames t mod 16), then u = (lam - mean) / max(norm, 1e-10) through a 64 x 64 LDS tile into the
//               bin-major copy (F, K, N): lanes on bins reading, lanes on frames writing.
//   tree level  four waves per (utterance, merge of two neighbouring groups), lanes on frames: the K x K float64 scores of the two
//               centroids, the best permutation p (one word per (level, merge)), the merged centroid into the other buffer.
//               A last odd group is copied up.  ceil(log2 F) launches; level 0 reads u itself.
//   compose     one thread per bin: pi_f = the product of the p on its path, bottom up.
//   refinement  per round: one workgroup per (utterance, class) sums u[f][pi_f[a]] over the bins in bin order and normalises
//               it (centroid); one wave per (utterance, bin) scores the bin against the centroids and updates pi_f (assign).
//   noise       one workgroup per utterance: the purity of every R_k[f], summed per stream; the smallest goes last.
//   finish      one wave per (utterance, bin): perm with the noise stream last, R (lanes on its elements) and log alpha gathered.
//   apply       one wave per (utterance, 32 frames, 64 bins): the masks gathered, lanes on bins.
#include <algorithm>

#include "array_internal.h"

namespace pk2 {

constexpr int kPaMaxK = PK2_BF_MAX_MASKS;
constexpr int kPaPart = PK2_BF_FRAMES_PER_PART;     // frames per workgroup of the apply pass
constexpr int kPaFeatWaves = 16;                    // waves of a feature workgroup: frames t mod 16
constexpr int kPaMergeWaves = 4;                    // waves of a merge workgroup: frames t mod 256
constexpr int kPaCentThreads = 1024;
constexpr int kPaNoiseThreads = 1024;
constexpr uint32_t kPaIdentity = 0x03020100u;
static_assert(kPaMaxK == 4, "a permutation is four bytes of one word");

struct PaTab {
  const float* lam[kArrayMaxUtts];
  float* out[kArrayMaxUtts];
  int64_t foff[kArrayMaxUtts];                      // frames of the call in front of this utterance
  Ragged rag;
};

__device__ __forceinline__ int pa_byte(uint32_t p, int a) { return (int)((p >> (8 * a)) & 3u); }

// (old o p)[a] = old[p[a]]
__device__ __forceinline__ uint32_t pa_compose(uint32_t old, uint32_t p, int K) {
  uint32_t r = kPaIdentity;
  for (int a = 0; a < K; ++a) r = (r & ~(0xffu << (8 * a))) | ((uint32_t)pa_byte(old, pa_byte(p, a)) << (8 * a));
  return r;
}

__device__ __forceinline__ double pa_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // a + b == b + a: every lane ends with the same bits
  return v;
}

// The permutation p maximising sum_a S[a][p[a]]: the K! candidates in lexicographic order, a later one replaces the best
// only on >.  top: its score; second: the largest score of the others.  Fully unrolled: S stays in registers.
template <int K>
__device__ __forceinline__ uint32_t pa_best(const double (&S)[K][K], double* top, double* second) {
  double bt = 0.0, sc = -INFINITY;
  uint32_t bp = kPaIdentity;
  bool have = false;
  constexpr int n2 = K > 2 ? K : 1, n3 = K > 3 ? K : 1;
#pragma unroll
  for (int p0 = 0; p0 < K; ++p0) {
#pragma unroll
    for (int p1 = 0; p1 < K; ++p1) {
      if (p1 == p0) continue;
#pragma unroll
      for (int p2 = 0; p2 < n2; ++p2) {
        if (K > 2 && (p2 == p0 || p2 == p1)) continue;
#pragma unroll
        for (int p3 = 0; p3 < n3; ++p3) {
          if (K > 3 && (p3 == p0 || p3 == p1 || p3 == p2)) continue;
          double s = S[0][p0] + S[1][p1];
          if (K > 2) s += S[2 % K][p2 % K];
          if (K > 3) s += S[3 % K][p3 % K];
          const uint32_t code = (uint32_t)p0 | ((uint32_t)p1 << 8) | ((K > 2 ? (uint32_t)p2 : 2u) << 16) |
                                ((K > 3 ? (uint32_t)p3 : 3u) << 24);
          if (!have) {
            bt = s; bp = code; have = true;
          } else if (s > bt) {
            sc = bt; bt = s; bp = code;
          } else if (s > sc) {
            sc = s;
          }
        }
      }
    }
  }
  *top = bt;
  *second = sc;
  return bp;
}

// grid (ceil(F / 64), K, utterances of the launch), block 64 kPaFeatWaves.  U: (F, K, N) per utterance at U + foff K F.
__global__ void __launch_bounds__(64 * kPaFeatWaves) pa_feature_kernel(const PaTab tab, int F, int K, float* __restrict__ U) {
  __shared__ double s_part[kPaFeatWaves][64];
  __shared__ float s_tile[64][65];
  const int b = blockIdx.z, k = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int N = tab.rag.frames[b];
  const int f0 = blockIdx.x * 64, f = f0 + lane;
  const bool live = f < F;
  const float* __restrict__ src = tab.lam[b] + (int64_t)k * N * F;
  float* __restrict__ dst = U + tab.foff[b] * K * F;
  double s = 0.0;
  if (live)
    for (int t = w; t < N; t += kPaFeatWaves) s += (double)src[(int64_t)t * F + f];
  s_part[w][lane] = s;
  __syncthreads();
  s = 0.0;
  for (int i = 0; i < kPaFeatWaves; ++i) s += s_part[i][lane];
  const double mean = s / (double)N;
  __syncthreads();
  s = 0.0;
  if (live)
    for (int t = w; t < N; t += kPaFeatWaves) {
      const double d = (double)src[(int64_t)t * F + f] - mean;
      s += d * d;
    }
  s_part[w][lane] = s;
  __syncthreads();
  s = 0.0;
  for (int i = 0; i < kPaFeatWaves; ++i) s += s_part[i][lane];
  const double den = fmax(sqrt(s), 1e-10);
  for (int t0 = 0; t0 < N; t0 += 64) {
    for (int r = w; r < 64; r += kPaFeatWaves) {
      const int t = t0 + r;
      s_tile[r][lane] = live && t < N ? (float)(((double)src[(int64_t)t * F + f] - mean) / den) : 0.f;
    }
    __syncthreads();
    for (int r = w; r < 64; r += kPaFeatWaves) {
      const int fb = f0 + r, t = t0 + lane;
      if (fb < F && t < N) dst[((int64_t)fb * K + k) * N + t] = s_tile[lane][r];
    }
    __syncthreads();
  }
}

// M sums over the kPaMergeWaves waves of a workgroup, the same bits in every thread: a butterfly per wave, the waves'
// results added in wave order.  s_red: kPaMergeWaves x M doubles, free again at the next call's first barrier.
template <int M>
__device__ __forceinline__ void pa_merge_sum(double (&v)[M], double* s_red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < M; ++i) v[i] = pa_wave_sum(v[i]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < M; ++i) s_red[w * M + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = 0.0;
    for (int k = 0; k < kPaMergeWaves; ++k) s += s_red[k * M + i];
    v[i] = s;
  }
}

// grid (groups of the next level, utterances of the launch), block 64 kPaMergeWaves.  src: the centroids of level `level`,
// (groups, K, N) per utterance at src + foff K srcF (level 0: u itself, srcF = F); dst: those of the next level at
// dst + foff K halfF.  tperm: (B, levels, halfF) words, this launch's utterances from tperm on.  Four passes over the two
// groups' rows, every one with the K classes' loads in flight together: scores, means, norms, the merged centroid.
template <int K>
__global__ void __launch_bounds__(64 * kPaMergeWaves) pa_merge_kernel(const PaTab tab, int F, int level, int levels, int halfF,
                                                                      int srcF, const float* __restrict__ src,
                                                                      float* __restrict__ dst, uint32_t* __restrict__ tperm) {
  constexpr int T = 64 * kPaMergeWaves;
  __shared__ double s_red[kPaMergeWaves * K * K];
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const int N = tab.rag.frames[b];
  const int groups = (F + (1 << level) - 1) >> level;
  const int64_t KN = (int64_t)K * N;
  const float* __restrict__ cL = src + tab.foff[b] * K * srcF + (int64_t)(2 * j) * KN;
  float* __restrict__ out = dst + tab.foff[b] * K * halfF + (int64_t)j * KN;
  if (2 * j + 1 >= groups) {                       // the last odd group passes up unchanged (the whole workgroup leaves)
    for (int64_t i = tid; i < KN; i += T) out[i] = cL[i];
    return;
  }
  const float* __restrict__ cR = cL + KN;
  double S[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) S[i] = 0.0;
  for (int t = tid; t < N; t += T) {
    double l[K], r[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      l[a] = (double)cL[(int64_t)a * N + t];
      r[a] = (double)cR[(int64_t)a * N + t];
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int c = 0; c < K; ++c) S[a * K + c] += l[a] * r[c];
  }
  pa_merge_sum<K * K>(S, s_red);
  double S2[K][K];
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int c = 0; c < K; ++c) S2[a][c] = S[a * K + c];
  double top, second;
  const uint32_t p = pa_best<K>(S2, &top, &second);
  if (tid == 0) tperm[((int64_t)b * levels + level) * halfF + j] = p;
  const double wL = (double)(1 << level), wR = (double)min(1 << level, F - ((2 * j + 1) << level));
  const float* y[K];
#pragma unroll
  for (int a = 0; a < K; ++a) y[a] = cR + (int64_t)pa_byte(p, a) * N;
  double mean[K], den[K];
#pragma unroll
  for (int a = 0; a < K; ++a) mean[a] = 0.0;
  for (int t = tid; t < N; t += T) {
#pragma unroll
    for (int a = 0; a < K; ++a) mean[a] += wL * (double)cL[(int64_t)a * N + t] + wR * (double)y[a][t];
  }
  pa_merge_sum<K>(mean, s_red);
#pragma unroll
  for (int a = 0; a < K; ++a) {
    mean[a] /= (double)N;
    den[a] = 0.0;
  }
  for (int t = tid; t < N; t += T) {
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const double d = (wL * (double)cL[(int64_t)a * N + t] + wR * (double)y[a][t]) - mean[a];
      den[a] += d * d;
    }
  }
  pa_merge_sum<K>(den, s_red);
#pragma unroll
  for (int a = 0; a < K; ++a) den[a] = fmax(sqrt(den[a]), 1e-10);
  for (int t = tid; t < N; t += T) {
#pragma unroll
    for (int a = 0; a < K; ++a)
      out[(int64_t)a * N + t] = (float)(((wL * (double)cL[(int64_t)a * N + t] + wR * (double)y[a][t]) - mean[a]) / den[a]);
  }
}

// grid (ceil(F / 64), utterances of the launch), block 64: pi_f = the product of the tree's p over the levels at which the
// bin sits in a right group, bottom up.  pi: (B, F) words.
__global__ void __launch_bounds__(64) pa_compose_kernel(int F, int K, int levels, int halfF, const uint32_t* __restrict__ tperm,
                                                        uint32_t* __restrict__ pi) {
  const int f = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (f >= F) return;
  uint32_t p = kPaIdentity;
  for (int l = 0; l < levels; ++l) {
    const int g = f >> l;
    if (g & 1) p = pa_compose(p, tperm[((int64_t)b * levels + l) * halfF + (g >> 1)], K);
  }
  pi[(int64_t)b * F + f] = p;
}

// sum over the kPaCentThreads threads of a workgroup, the same bits in every thread; s_w: 16 doubles
__device__ __forceinline__ double pa_block_sum(double v, double* s_w) {
  v = pa_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < kPaCentThreads / 64; ++i) s += s_w[i];
  return s;
}

// grid (K, utterances of the launch), block kPaCentThreads: c[a] = pearson(sum_f u[f][pi_f[a]]), the bins in order.
// csum: float64 (K, N) per utterance at csum + foff K; cent: float32 the same.
__global__ void __launch_bounds__(kPaCentThreads) pa_centroid_kernel(const PaTab tab, int F, int K, const float* __restrict__ U,
                                                                     const uint32_t* __restrict__ pi, double* __restrict__ csum,
                                                                     float* __restrict__ cent) {
  __shared__ double s_w[kPaCentThreads / 64];
  const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int N = tab.rag.frames[b];
  const float* __restrict__ u = U + tab.foff[b] * K * F;
  const uint32_t* __restrict__ p = pi + (int64_t)b * F;
  double* __restrict__ cs = csum + (tab.foff[b] * K + (int64_t)a * N);
  float* __restrict__ c = cent + (tab.foff[b] * K + (int64_t)a * N);
  double tot = 0.0;
  for (int t = tid; t < N; t += kPaCentThreads) {
    double s = 0.0;
#pragma unroll 8
    for (int f = 0; f < F; ++f) s += (double)u[((int64_t)f * K + pa_byte(p[f], a)) * N + t];
    cs[t] = s;
    tot += s;
  }
  const double mean = pa_block_sum(tot, s_w) / (double)N;
  tot = 0.0;
  for (int t = tid; t < N; t += kPaCentThreads) {      // a thread reads back what it wrote itself
    const double d = cs[t] - mean;
    tot += d * d;
  }
  const double den = fmax(sqrt(pa_block_sum(tot, s_w)), 1e-10);
  for (int t = tid; t < N; t += kPaCentThreads) c[t] = (float)((cs[t] - mean) / den);
}

// grid (F, utterances of the launch), block 64: S[a][c] = <cent[a], u[f][pi_f[c]]>, p = best(S), pi_f <- pi_f o p; in the
// last round margin[f] = the best score - the second best.  margin: (B, F).
template <int K>
__global__ void __launch_bounds__(64) pa_assign_kernel(const PaTab tab, int F, const float* __restrict__ U,
                                                       const float* __restrict__ cent, uint32_t* __restrict__ pi,
                                                       float* __restrict__ margin) {
  const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int N = tab.rag.frames[b];
  const uint32_t old = pi[(int64_t)b * F + f];
  const float* __restrict__ c = cent + tab.foff[b] * K;
  const float* __restrict__ u = U + tab.foff[b] * K * F + (int64_t)f * K * N;
  const float* row[K];
#pragma unroll
  for (int a = 0; a < K; ++a) row[a] = u + (int64_t)pa_byte(old, a) * N;
  double S[K][K];
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int k = 0; k < K; ++k) S[a][k] = 0.0;
  for (int t = lane; t < N; t += 64) {
    double l[K], r[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      l[a] = (double)c[(int64_t)a * N + t];
      r[a] = (double)row[a][t];
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int k = 0; k < K; ++k) S[a][k] += l[a] * r[k];
  }
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int k = 0; k < K; ++k) S[a][k] = pa_wave_sum(S[a][k]);
  double top, second;
  const uint32_t p = pa_best<K>(S, &top, &second);
  if (lane == 0) {
    pi[(int64_t)b * F + f] = pa_compose(old, p, K);
    if (margin) margin[(int64_t)b * F + f] = (float)(top - second);
  }
}

// grid (utterances of the launch), block kPaNoiseThreads: q[a] = sum_f ||R||_F^2 / (Re tr R)^2 of R[pi_f[a]][f] over the
// bins where it is finite; noise[b] = the stream with the smallest q (a tie keeps the first).  R: (B, K, F, C, C);
// pur: (B, K, F) float64.
__global__ void __launch_bounds__(kPaNoiseThreads) pa_noise_kernel(int C, int F, int K, const float2* __restrict__ R,
                                                                   const uint32_t* __restrict__ pi, double* __restrict__ pur,
                                                                   int32_t* __restrict__ noise) {
  __shared__ double s_q[kPaMaxK][kPaNoiseThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  double* __restrict__ pu = pur + (int64_t)b * K * F;
  for (int i = tid; i < K * F; i += kPaNoiseThreads) {
    const float2* __restrict__ M = R + ((int64_t)b * K * F + i) * C * C;
    double fro = 0.0, tr = 0.0;
    for (int r = 0; r < C; ++r)
      for (int c = 0; c < C; ++c) {
        const float2 v = M[r * C + c];
        fro += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        if (r == c) tr += (double)v.x;
      }
    pu[i] = fro / (tr * tr);
  }
  __syncthreads();
  for (int a = 0; a < K; ++a) {
    double q = 0.0;
    for (int f = tid; f < F; f += kPaNoiseThreads) {
      const double v = pu[(int64_t)pa_byte(pi[(int64_t)b * F + f], a) * F + f];
      if (isfinite(v)) q += v;
    }
    q = pa_wave_sum(q);
    if ((tid & 63) == 0) s_q[a][tid >> 6] = q;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    double qb = 0.0;
    for (int a = 0; a < K; ++a) {
      double q = 0.0;
      for (int i = 0; i < kPaNoiseThreads / 64; ++i) q += s_q[a][i];
      if (a == 0 || q < qb) { qb = q; best = a; }
    }
    noise[b] = best;
  }
}

// grid (F, utterances of the launch), block 64: perm (B, F, K) of the bin with the noise stream (noise[b], or none) moved
// last, and R (B, K, F, C, C) and log_alpha (B, K, F) gathered by it (null: none), the lanes on the elements of a matrix.
__global__ void __launch_bounds__(64) pa_finish_kernel(int C, int F, int K, const uint32_t* __restrict__ pi,
                                                       const int32_t* __restrict__ noise, const float2* __restrict__ R,
                                                       const float* __restrict__ la, int32_t* __restrict__ perm,
                                                       float2* __restrict__ out_R, float* __restrict__ out_la) {
  const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const uint32_t p = pi[(int64_t)b * F + f];
  const int ns = noise ? noise[b] : K - 1;
  for (int a = 0; a < K; ++a) {
    const int from = pa_byte(p, a < K - 1 ? (a < ns ? a : a + 1) : ns);
    if (lane == 0) perm[((int64_t)b * F + f) * K + a] = from;
    if (R) {
      const float2* __restrict__ s = R + (((int64_t)b * K + from) * F + f) * C * C;
      float2* __restrict__ d = out_R + (((int64_t)b * K + a) * F + f) * C * C;
      for (int e = lane; e < C * C; e += 64) d[e] = s[e];
      if (lane == 0) out_la[((int64_t)b * K + a) * F + f] = la[((int64_t)b * K + from) * F + f];
    }
  }
}

// grid (parts of the launch, ceil(F / 64)), block 64: out[a, t, f] = lam[perm[f][a], t, f].  perm: this launch's, (nb, F, K).
__global__ void __launch_bounds__(64) pa_apply_kernel(const PaTab tab, int B, int F, int K, const int32_t* __restrict__ perm) {
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * 64 + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kPaPart, t1 = min(t0 + kPaPart, N);
  const int64_t NF = (int64_t)N * F;
  const float* __restrict__ src = tab.lam[b];
  float* __restrict__ dst = tab.out[b];
  int64_t from[kPaMaxK];
#pragma unroll
  for (int a = 0; a < kPaMaxK; ++a) from[a] = a < K ? perm[((int64_t)b * F + f) * K + a] * NF : 0;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
#pragma unroll
    for (int a = 0; a < kPaMaxK; ++a)
      if (a < K) dst[a * NF + o] = src[from[a] + o];
  }
}

static int pa_levels(int F) {
  int l = 0;
  while (((F + (1 << l) - 1) >> l) > 1) ++l;
  return l;
}

struct PaWork {
  float *u, *cent0, *cent1, *c;
  double *csum, *pur;
  uint32_t *pi, *tperm;
  int32_t* noise;
  size_t bytes;
};

static PaWork pa_carve(void* base, const int32_t* frames, int32_t B, int32_t F, int32_t K) {
  int64_t total = 0;
  for (int b = 0; b < B; ++b) total += frames[b];
  const int halfF = (F + 1) / 2, levels = std::max(pa_levels(F), 1);
  Carver cv(base);
  PaWork w;
  w.u = cv.take<float>((size_t)total * K * F);
  w.cent0 = cv.take<float>((size_t)total * K * halfF);
  w.cent1 = cv.take<float>((size_t)total * K * halfF);
  w.csum = cv.take<double>((size_t)total * K);
  w.c = cv.take<float>((size_t)total * K);
  w.pur = cv.take<double>((size_t)B * K * F);
  w.pi = cv.take<uint32_t>((size_t)B * F);
  w.tperm = cv.take<uint32_t>((size_t)B * levels * halfF);
  w.noise = cv.take<int32_t>((size_t)B);
  w.bytes = cv.bytes();
  return w;
}

template <int K>
static void pa_tree_and_refine(const PaTab& tab, int nb, int F, int levels, int refine, const PaWork& w, int b0, float* margin,
                               hipStream_t stream) {
  const int halfF = (F + 1) / 2;
  const unsigned tiles = (unsigned)((F + 63) / 64);
  uint32_t* tperm = w.tperm + (int64_t)b0 * std::max(levels, 1) * halfF;
  uint32_t* pi = w.pi + (int64_t)b0 * F;
  for (int l = 0; l < levels; ++l) {
    const int groups = (F + (1 << l) - 1) >> l;
    const float* src = l == 0 ? w.u : (l & 1) ? w.cent0 : w.cent1;
    float* dst = (l & 1) ? w.cent1 : w.cent0;
    hipLaunchKernelGGL(pa_merge_kernel<K>, dim3((unsigned)((groups + 1) / 2), (unsigned)nb), dim3(64 * kPaMergeWaves), 0,
                       stream, tab, F, l, levels, halfF, l == 0 ? F : halfF, src, dst, tperm);
  }
  hipLaunchKernelGGL(pa_compose_kernel, dim3(tiles, (unsigned)nb), dim3(64), 0, stream, F, K, levels, halfF, tperm, pi);
  for (int r = 0; r < refine; ++r) {
    hipLaunchKernelGGL(pa_centroid_kernel, dim3((unsigned)K, (unsigned)nb), dim3(kPaCentThreads), 0, stream, tab, F, K, w.u, pi,
                       w.csum, w.c);
    hipLaunchKernelGGL(pa_assign_kernel<K>, dim3((unsigned)F, (unsigned)nb), dim3(64), 0, stream, tab, F, w.u, w.c, pi,
                       r == refine - 1 ? margin : (float*)nullptr);
  }
}

}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_perm_align_workspace_bytes(const int32_t* frames, int32_t B, int32_t F, int32_t K) {
  if (!frames || B < 1 || B > 8192 || F < 1 || F > 4097 || K < 2 || K > PK2_BF_MAX_MASKS) return 0;
  for (int b = 0; b < B; ++b)
    if (frames[b] < 1 || frames[b] > (1 << 24)) return 0;
  return pa_carve(nullptr, frames, B, F, K).bytes;
}

extern "C" int pk2_perm_align(const float* const* masks, const float* cov, const float* log_alpha, const int32_t* frames,
                              int32_t B, int32_t C, int32_t F, int32_t K, int32_t refine, int32_t noise_last, void* work,
                              size_t work_bytes, float* const* out_masks, float* out_cov, float* out_log_alpha, int32_t* perm,
                              float* margin, void* stream_) {
  PK2_REQUIRE(B >= 1 && B <= 8192, "perm_align: %d utterances (1 to 8192)", B);
  PK2_REQUIRE(F >= 1 && F <= 4097, "perm_align: %d bins (1 to 4097)", F);
  PK2_REQUIRE(K >= 2 && K <= PK2_BF_MAX_MASKS, "perm_align: %d classes (2 to %d)", K, PK2_BF_MAX_MASKS);
  PK2_REQUIRE(refine >= 1 && refine <= PK2_PERM_ALIGN_MAX_REFINE, "perm_align: %d refinement rounds (1 to %d)", refine,
              PK2_PERM_ALIGN_MAX_REFINE);
  PK2_REQUIRE(work && perm && margin, "perm_align: null pointer");
  PK2_REQUIRE((cov != nullptr) == (log_alpha != nullptr) && (cov != nullptr) == (out_cov != nullptr) &&
                  (cov != nullptr) == (out_log_alpha != nullptr),
              "perm_align: cov, log_alpha, out_cov and out_log_alpha are given together or not at all");
  if (cov) PK2_REQUIRE(C >= 1 && C <= PK2_BF_MAX_CHANNELS, "perm_align: %d channels (1 to %d)", C, PK2_BF_MAX_CHANNELS);
  PK2_REQUIRE(cov != out_cov || !cov, "perm_align: the covariances are permuted out of place");
  PK2_REQUIRE(log_alpha != out_log_alpha || !log_alpha, "perm_align: log_alpha is permuted out of place");
  if (int rc = check_frames("perm_align", frames, B)) return rc;
  if (int rc = check_table("perm_align", "the masks", masks, B)) return rc;
  if (int rc = check_table("perm_align", "the aligned masks", out_masks, B)) return rc;
  for (int b = 0; b < B; ++b)
    PK2_REQUIRE(masks[b] != out_masks[b], "perm_align: utterance %d: the masks are permuted out of place", b);
  const PaWork w = pa_carve(work, frames, B, F, K);
  PK2_REQUIRE(work_bytes >= w.bytes, "perm_align: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int levels = pa_levels(F);
  const unsigned tiles = (unsigned)((F + 63) / 64);
  const bool noise = cov && noise_last;
  int64_t frame_off = 0;
  for (int b0 = 0; b0 < B; b0 += kArrayMaxUtts) {
    const int nb = std::min<int>(kArrayMaxUtts, B - b0);
    PaTab tab;
    memset(&tab, 0, sizeof(tab));
    int64_t parts;
    if (int rc = fill_ragged("perm_align", tab.rag, frames, b0, nb, kPaPart, &parts)) return rc;
    for (int b = 0; b < nb; ++b) {
      tab.lam[b] = masks[b0 + b];
      tab.out[b] = out_masks[b0 + b];
      tab.foff[b] = frame_off;
      frame_off += frames[b0 + b];
    }
    hipLaunchKernelGGL(pa_feature_kernel, dim3(tiles, (unsigned)K, (unsigned)nb), dim3(64 * kPaFeatWaves), 0, stream, tab, F, K,
                       w.u);
    PK2_LAUNCH_CHECK();
    float* mg = margin + (int64_t)b0 * F;
    if (K == 2) pa_tree_and_refine<2>(tab, nb, F, levels, refine, w, b0, mg, stream);
    else if (K == 3) pa_tree_and_refine<3>(tab, nb, F, levels, refine, w, b0, mg, stream);
    else pa_tree_and_refine<4>(tab, nb, F, levels, refine, w, b0, mg, stream);
    PK2_LAUNCH_CHECK();
    const int64_t kf = (int64_t)b0 * K * F;
    const float2* Rb = cov ? reinterpret_cast<const float2*>(cov) + kf * C * C : nullptr;
    if (noise) {
      hipLaunchKernelGGL(pa_noise_kernel, dim3((unsigned)nb), dim3(kPaNoiseThreads), 0, stream, C, F, K, Rb, w.pi + (int64_t)b0 * F,
                         w.pur + kf, w.noise + b0);
      PK2_LAUNCH_CHECK();
    }
    int32_t* pm = perm + (int64_t)b0 * F * K;
    hipLaunchKernelGGL(pa_finish_kernel, dim3((unsigned)F, (unsigned)nb), dim3(64), 0, stream, C, F, K, w.pi + (int64_t)b0 * F,
                       noise ? w.noise + b0 : (const int32_t*)nullptr, Rb, cov ? log_alpha + kf : nullptr, pm,
                       cov ? reinterpret_cast<float2*>(out_cov) + kf * C * C : nullptr, cov ? out_log_alpha + kf : nullptr);
    PK2_LAUNCH_CHECK();
    hipLaunchKernelGGL(pa_apply_kernel, dim3((unsigned)parts, tiles), dim3(64), 0, stream, tab, nb, F, K, pm);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}
