// The array front end: what csrc/beamform.hip, csrc/cgmm.hip and csrc/wpe.hip share.
//
//   host     check_shape / check_frames / check_table, the ragged-launch header Ragged with fill_ragged, dispatch_channels
//   device   find_utt, the complex double cd, hermitian_cholesky (per thread, float64), any_flag_kernel
//   kernels  cov_kernel<C, Weights> and cov_reduce_kernel: the weighted spatial covariance pass.  Lanes on bins, one wave per
//            (utterance, PK2_BF_FRAMES_PER_PART frames, 64 bins): the spectrum is read once, coalesced along f, for all weight
//            planes; the C (C + 1) / 2 complex sums per plane and the normalisers live in registers and go to the workspace as
//            one partial per part.  The reduce kernel adds the partials in part order in float64, divides by the normaliser
//            and writes both triangles.  No atomics: a result depends on its utterance alone.  beamform.hip weighs with masks,
//            cgmm.hip with posteriors (its M-step); each defines its Weights next to its launch table.
#pragma once
#include <type_traits>

#include "common.h"

namespace pk2 {

static_assert(PK2_WPE_MAX_UTTS == PK2_BF_MAX_UTTS, "one launch header for the three sources");
static_assert(PK2_WPE_MAX_CHANNELS == 8 && PK2_BF_MAX_CHANNELS == 8, "dispatch_channels and check_shape cover 1 to 8 channels");

constexpr int kArrayMaxUtts = PK2_BF_MAX_UTTS;      // utterances per launch
constexpr int kCovLanes = 64;                       // bins per workgroup (one wave) of the covariance pass
constexpr int kCovPart = PK2_BF_FRAMES_PER_PART;    // frames per workgroup of the covariance pass

__host__ __device__ constexpr int tri_pairs(int C) { return C * (C + 1) / 2; }
// floats of one (part, plane) partial per bin: the lower triangle (re, im) row by row, then the normaliser
__host__ __device__ constexpr int cov_entries(int C) { return 2 * tri_pairs(C) + 1; }

// The header of a ragged launch table: a workgroup's blockIdx.x is a part (a run of frames) of one utterance.
struct Ragged {
  int32_t frames[kArrayMaxUtts];
  int32_t part_off[kArrayMaxUtts + 1];              // first part of every utterance in this launch
};

// fills the header for utterances [b0, b0 + nb) at per_part frames per part; *parts: the parts of the launch
static inline int fill_ragged(const char* who, Ragged& r, const int32_t* frames, int b0, int nb, int per_part, int64_t* parts) {
  int64_t n = 0;
  for (int b = 0; b < nb; ++b) {
    r.frames[b] = frames[b0 + b];
    r.part_off[b] = (int32_t)n;
    n += ((int64_t)frames[b0 + b] + per_part - 1) / per_part;
    PK2_REQUIRE(n <= INT32_MAX / 2, "%s: too many frames in one launch", who);
  }
  for (int b = nb; b <= kArrayMaxUtts; ++b) r.part_off[b] = (int32_t)n;
  *parts = n;
  return PK2_OK;
}

static inline int check_shape(const char* who, int32_t B, int32_t C, int32_t F) {
  PK2_REQUIRE(B >= 1, "%s: no utterance (B = %d)", who, B);
  PK2_REQUIRE(C >= 1 && C <= PK2_BF_MAX_CHANNELS, "%s: %d channels (1 to %d)", who, C, PK2_BF_MAX_CHANNELS);
  PK2_REQUIRE(F >= 1 && F <= 4097, "%s: %d bins (1 to 4097)", who, F);
  return PK2_OK;
}

static inline int check_frames(const char* who, const int32_t* frames, int32_t B) {
  PK2_REQUIRE(frames, "%s: frames is null", who);
  for (int b = 0; b < B; ++b)
    PK2_REQUIRE(frames[b] >= 1 && frames[b] <= (1 << 24), "%s: utterance %d has %d frames (1 to 2^24)", who, b, frames[b]);
  return PK2_OK;
}

template <typename T>
int check_table(const char* who, const char* what, T* const* p, int32_t B) {
  PK2_REQUIRE(p, "%s: %s is null", who, what);
  for (int b = 0; b < B; ++b) PK2_REQUIRE(p[b], "%s: %s of utterance %d is null", who, what, b);
  return PK2_OK;
}

// Calls f(std::integral_constant<int, C>) for the channel count of a call (check_shape has seen it).
template <typename F>
void dispatch_channels(int C, F&& f) {
  switch (C) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

__device__ __forceinline__ int find_utt(const int32_t (&off)[kArrayMaxUtts + 1], int n, int part) {
  int b = 0;
  while (b + 1 < n && off[b + 1] <= part) ++b;
  return b;
}

struct cd {
  double x, y;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd cmulc(cd a, cd b) { return cd{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }   // a conj(b)
__device__ __forceinline__ cd cdivc(cd a, cd b) {
  const double d = b.x * b.x + b.y * b.y;
  return cd{(a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d};
}

// One thread, float64, A a C x C Hermitian block the caller has loaded: A += load I, then the Cholesky A = L L^H in the lower
// triangle of A.  ok: whether the caller's inputs were finite (false skips the factorisation); it becomes false where A is
// not positive definite.  logdet, when given, gets sum log L_jj.  The callers keep their load loops: bf_weights_kernel loads
// its two blocks in one statement, and with the load in here it measured 4 to 6 % slower.
__device__ __forceinline__ void hermitian_cholesky(cd (&A)[PK2_BF_MAX_CHANNELS][PK2_BF_MAX_CHANNELS], int C, double load, bool& ok,
                                                   double* logdet = nullptr) {
  for (int i = 0; i < C; ++i) { A[i][i].x += load; A[i][i].y = 0.0; }
  for (int j = 0; j < C && ok; ++j) {
    double d = A[j][j].x;
    for (int k = 0; k < j; ++k) d -= A[j][k].x * A[j][k].x + A[j][k].y * A[j][k].y;
    if (!(d > 0.0) || !isfinite(d)) { ok = false; break; }
    const double l = sqrt(d), inv = 1.0 / l;
    if (logdet) *logdet += log(l);
    A[j][j] = cd{l, 0.0};
    for (int i = j + 1; i < C; ++i) {
      cd s = A[i][j];
      for (int k = 0; k < j; ++k) { const cd q = cmulc(A[i][k], A[j][k]); s.x -= q.x; s.y -= q.y; }
      A[i][j] = cd{s.x * inv, s.y * inv};
    }
  }
}

// grid (utterances), block THREADS: nonfinite[b] = any of the utterance's count flags.  (This and cov_reduce_kernel are
// templates so that only the sources that launch them carry a copy.)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) any_flag_kernel(const int32_t* __restrict__ bad, int count,
                                                           int32_t* __restrict__ nonfinite) {
  const int b = blockIdx.x;
  int any = 0;
  for (int i = threadIdx.x; i < count; i += THREADS) any |= bad[(int64_t)b * count + i];
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) nonfinite[b] = any ? 1 : 0;
}

// grid (parts of the launch, ceil(F / 64)).  Weights: KA planes; Tab with spec[] and the header rag; built once per thread
// from (tab, b), its load(o, NF, m, ms) gives the weights m[k] of the frame at offset o and adds its normaliser terms to ms[k].
// partial layout: [part][KA][cov_entries(C)][F] float32
// amdgpu_waves_per_eu(1, 2): without it the register allocator aims at the occupancy of a 64-lane workgroup's default
// budget and spills 100 to 340 bytes per lane to scratch for C = 5 .. 7; with it every instantiation is scratch-free
// (C = 8 with four planes keeps its sums partly in AGPRs).  Small C still get the occupancy their register count allows.
template <int C, typename Weights>
__global__ void __launch_bounds__(kCovLanes) __attribute__((amdgpu_waves_per_eu(1, 2)))
cov_kernel(const typename Weights::Tab tab, int B, int F, float* __restrict__ work) {
  constexpr int KA = Weights::KA;
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * kCovLanes + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kCovPart, t1 = min(t0 + kCovPart, N);
  const float2* __restrict__ Y = tab.spec[b];
  const Weights W(tab, b);

  float re[KA][tri_pairs(C)], im[KA][tri_pairs(C)], ms[KA];
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    ms[k] = 0.f;
#pragma unroll
    for (int p = 0; p < tri_pairs(C); ++p) re[k][p] = im[k][p] = 0.f;
  }
  const int64_t NF = (int64_t)N * F;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
    float2 y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = Y[c * NF + o];
    float m[KA];
    W.load(o, NF, m, ms);
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j, ++p) {
        // y_i conj(y_j)
        const float pr = fmaf(y[i].x, y[j].x, y[i].y * y[j].y);
        const float pi = fmaf(y[i].y, y[j].x, -(y[i].x * y[j].y));
#pragma unroll
        for (int k = 0; k < KA; ++k) {
          re[k][p] = fmaf(m[k], pr, re[k][p]);
          if (i != j) im[k][p] = fmaf(m[k], pi, im[k][p]);
        }
      }
    }
  }
  constexpr int E = cov_entries(C);
  float* __restrict__ dst = work + (int64_t)part * KA * E * F + f;
#pragma unroll
  for (int k = 0; k < KA; ++k) {
#pragma unroll
    for (int p = 0; p < tri_pairs(C); ++p) {
      dst[(int64_t)(k * E + 2 * p) * F] = re[k][p];
      dst[(int64_t)(k * E + 2 * p + 1) * F] = im[k][p];
    }
    dst[(int64_t)(k * E + E - 1) * F] = ms[k];
  }
}

// grid (ceil(F / 64), pairs, utterances of the launch * KA): one element of the lower triangle and its mirror image.
// phi: (nb, KA, F, C, C).  With log_alpha (nb, KA, F) and nact (nb), the workgroups of element 0 also write
// log max(normaliser / max(nact, 1), 1e-10).
template <typename Tab>
__global__ void __launch_bounds__(kCovLanes) cov_reduce_kernel(const Tab tab, int C, int KA, int F, const float* __restrict__ work,
                                                               float2* __restrict__ phi, const int32_t* __restrict__ nact,
                                                               float* __restrict__ log_alpha) {
  const int f = blockIdx.x * kCovLanes + threadIdx.x;
  if (f >= F) return;
  const int p = blockIdx.y, b = blockIdx.z / KA, k = blockIdx.z % KA;
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  const int j = p - i * (i + 1) / 2;
  const int E = cov_entries(C);
  const int part0 = tab.rag.part_off[b], part1 = tab.rag.part_off[b + 1];
  double sr = 0.0, si = 0.0, sm = 0.0;
  for (int part = part0; part < part1; ++part) {
    const float* __restrict__ src = work + ((int64_t)part * KA + k) * E * F + f;
    sr += (double)src[(int64_t)(2 * p) * F];
    si += (double)src[(int64_t)(2 * p + 1) * F];
    sm += (double)src[(int64_t)(E - 1) * F];
  }
  const double den = fmax(sm, 1e-10);
  const float vr = (float)(sr / den), vi = i == j ? 0.f : (float)(si / den);
  float2* __restrict__ out = phi + (((int64_t)b * KA + k) * F + f) * C * C;
  out[i * C + j] = make_float2(vr, vi);
  if (i != j) out[j * C + i] = make_float2(vr, -vi);
  if (log_alpha && p == 0) log_alpha[((int64_t)b * KA + k) * F + f] = (float)log(fmax(sm / (double)max(nact[b], 1), 1e-10));
}

// the covariance pass of one launch: partials into work, then phi (and log_alpha) of its nb utterances
template <int C, typename Weights>
void cov_launch(const typename Weights::Tab& tab, int nb, int64_t parts, int F, float* work, float2* phi, const int32_t* nact,
                float* log_alpha, hipStream_t stream) {
  const unsigned tiles = (unsigned)((F + kCovLanes - 1) / kCovLanes);
  hipLaunchKernelGGL((cov_kernel<C, Weights>), dim3((unsigned)parts, tiles), dim3(kCovLanes), 0, stream, tab, nb, F, work);
  hipLaunchKernelGGL(cov_reduce_kernel<typename Weights::Tab>, dim3(tiles, (unsigned)tri_pairs(C), (unsigned)(nb * Weights::KA)),
                     dim3(kCovLanes), 0, stream, tab, C, Weights::KA, F, work, phi, nact, log_alpha);
}

}  // namespace pk2
