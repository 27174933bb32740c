// WPE dereverberation for a ragged minibatch (include/pk2hip.h): multi-channel linear prediction per bin.
//
//   pk2_wpe_power    lanes on bins: max(sum_c |Y|^2 / C, 1e-10), one pass over the spectrum.
//   pk2_wpe_corr     a pre-pass copies the spectrum bin-major ((f, c, t): the frame series of a bin becomes contiguous) and
//                    the reciprocal weights as (f, t).  One workgroup per (utterance, part of PK2_WPE_FRAMES_PER_PART frames,
//                    bin) stages 64 frames and their past in LDS; the E = D + C complex rows [y~; Y] form up to three tiles
//                    of 32, and every wave owns one pair of tiles (I >= J) of the lower triangle of [y~; Y] diag(1/w) [y~; Y]^H:
//                    two accumulators (re, im) fed by four mfma_f32_32x32x2f32 per two frames, re += ar br + ai bi,
//                    im += ai br - ar bi, the weighted rows on the A side.  Row (k, c) at frame t is a shifted read of the
//                    staged frames; the stacked matrix is never built.  A second kernel adds the parts in part order in
//                    float64, rounds once and writes R with its mirror image and P = conj of the (Y, y~) block.
//   pk2_wpe_solve    one workgroup per (utterance, bin): R' as a packed lower triangle of complex128 in LDS (52 KB at order
//                    80) and P beside it, right-looking Cholesky in place, forward and back substitution column-oriented,
//                    every element's updates in ascending order; the finite checks and the per-bin flag.
//   pk2_wpe_filter   lanes on bins, 8 bins x 32 thread rows x 4 consecutive frames: the G of the 8 bins in LDS, the past of the
//                    4 frames a sliding window in registers, fmaf chains in ascending d; the power of the result from the same
//                    registers.  A bin whose G is all zero is copied.
//   pk2_wpe          the iterations: the bin-major spectrum is made once, the intermediate iterations write only the power.
//
// The ragged-launch header and its fill, the argument checks, find_utt, the complex double, any_flag_kernel and
// dispatch_channels are array_internal.h's, shared with beamform.hip and cgmm.hip.
#include <algorithm>

#include "array_internal.h"

namespace pk2 {

typedef float wpe_f16 __attribute__((ext_vector_type(16)));

constexpr int kWpePart = PK2_WPE_FRAMES_PER_PART;   // frames per workgroup of the correlation pass
constexpr int kWpeChunk = 64;                       // frames staged in LDS at a time
constexpr int kWpeStage = 656;                      // >= C (64 + delay + K - 1) for every allowed (C, K, delay): 8 * 81
constexpr int kWpeMaxPairs = 6;                     // tile pairs of the lower triangle of 3 x 3 tiles
constexpr int kWpeFB = 8, kWpeFR = 32, kWpeTF = 4;  // filter: bins, thread rows, consecutive frames per thread
constexpr int kWpeFilterFrames = kWpeFR * kWpeTF;
constexpr int kWpeTri = PK2_WPE_MAX_ORDER * (PK2_WPE_MAX_ORDER + 1) / 2;

struct WpeTab {
  const float2* spec[PK2_WPE_MAX_UTTS];
  const float* weight[PK2_WPE_MAX_UTTS];
  float2* out[PK2_WPE_MAX_UTTS];
  float* power[PK2_WPE_MAX_UTTS];
  int64_t yoff[PK2_WPE_MAX_UTTS];                   // float2 offset of the utterance's (F, C, N) copy
  int64_t woff[PK2_WPE_MAX_UTTS];                   // float offset of its (F, N) reciprocal weights
  Ragged rag;
};

__host__ __device__ constexpr int wpe_tiles(int E) { return (E + 31) / 32; }
__host__ __device__ constexpr int wpe_pairs(int E) { return wpe_tiles(E) * (wpe_tiles(E) + 1) / 2; }

// grid (parts of 32 frames, ceil(F / 64)): tab.power[b][t, f]
__global__ void __launch_bounds__(64) wpe_power_kernel(const WpeTab tab, int B, int C, int F) {
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int f = blockIdx.y * 64 + threadIdx.x;
  if (f >= F) return;
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * 32, t1 = min(t0 + 32, N);
  const float2* __restrict__ Y = tab.spec[b];
  float* __restrict__ pw = tab.power[b];
  const int64_t NF = (int64_t)N * F;
  const float fc = (float)C;
  for (int t = t0; t < t1; ++t) {
    const int64_t o = (int64_t)t * F + f;
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float2 y = Y[c * NF + o];
      s = fmaf(y.x, y.x, s);
      s = fmaf(y.y, y.y, s);
    }
    pw[o] = fmaxf(s / fc, 1e-10f);
  }
}

// grid (parts of 32 frames, ceil(F / 32), planes), block 256 = 32 x 8.  Planes: the C channels of the spectrum when
// do_spec, then the weight when do_weight.  (C, N, F) -> yt (F, C, N); (N, F) -> wt (F, N) = 1 / weight.
__global__ void __launch_bounds__(256) wpe_transpose_kernel(const WpeTab tab, int B, int C, int F, int do_spec,
                                                            float2* __restrict__ yt, float* __restrict__ wt) {
  __shared__ float2 tile[32][33];
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int plane = blockIdx.z;
  const bool is_spec = do_spec && plane < C;
  if (is_spec) {
    const float2* __restrict__ Y = tab.spec[b] + (int64_t)plane * N * F;
    for (int r = ty; r < 32; r += 8) {
      const int t = t0 + r, f = f0 + tx;
      if (t < N && f < F) tile[r][tx] = Y[(int64_t)t * F + f];
    }
  } else {
    const float* __restrict__ W = tab.weight[b];
    for (int r = ty; r < 32; r += 8) {
      const int t = t0 + r, f = f0 + tx;
      if (t < N && f < F) tile[r][tx] = make_float2(1.0f / W[(int64_t)t * F + f], 0.f);
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int f = f0 + r, t = t0 + tx;
    if (t < N && f < F) {
      if (is_spec) yt[tab.yoff[b] + ((int64_t)f * C + plane) * N + t] = tile[tx][r];
      else wt[tab.woff[b] + (int64_t)f * N + t] = tile[tx][r].x;
    }
  }
}

// grid (parts of the launch, F), block 64 * pairs.  partial layout: [part][f][pair][re, im][32][32] float32
__global__ void __launch_bounds__(64 * kWpeMaxPairs) wpe_corr_kernel(const WpeTab tab, int B, int C, int F, int K, int delay,
                                                                     const float2* __restrict__ yt,
                                                                     const float* __restrict__ wt,
                                                                     float* __restrict__ parts) {
  __shared__ float2 ys[kWpeStage];
  __shared__ float ws[kWpeChunk];
  const int part = blockIdx.x, f = blockIdx.y;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int N = tab.rag.frames[b];
  const int t0 = (part - tab.rag.part_off[b]) * kWpePart, t1 = min(t0 + kWpePart, N);
  const int D = C * K, E = D + C;
  const int halo = delay + K - 1, LW = kWpeChunk + halo;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
  const int I = wave >= 3 ? 2 : (wave >= 1 ? 1 : 0), J = wave - I * (I + 1) / 2;
  // the staged position of row e at local frame 0: channel c, shifted back by delay + k (y~) or by 0 (Y).  Rows past E read
  // position 0: their products land in elements nobody reads.
  int abase = 0, bbase = 0;
  {
    const int i = I * 32 + r, j = J * 32 + r;
    if (i < D) abase = (i % C) * LW + halo - (delay + i / C);
    else if (i < E) abase = (i - D) * LW + halo;
    if (j < D) bbase = (j % C) * LW + halo - (delay + j / C);
    else if (j < E) bbase = (j - D) * LW + halo;
  }
  const float2* __restrict__ Yb = yt + tab.yoff[b] + (int64_t)f * C * N;
  const float* __restrict__ Wb = wt + tab.woff[b] + (int64_t)f * N;
  wpe_f16 re, im;
#pragma unroll
  for (int v = 0; v < 16; ++v) re[v] = im[v] = 0.f;
  for (int tc = t0; tc < t1; tc += kWpeChunk) {
    __syncthreads();
    for (int p = tid; p < C * LW; p += nthreads) {
      const int c = p / LW, q = p - c * LW;
      const int t = tc - halo + q;
      ys[p] = (t >= 0 && t < N) ? Yb[(int64_t)c * N + t] : make_float2(0.f, 0.f);
    }
    for (int q = tid; q < kWpeChunk; q += nthreads) ws[q] = tc + q < t1 ? Wb[tc + q] : 0.f;
    __syncthreads();
    const int steps = (min(kWpeChunk, t1 - tc) + 1) >> 1;
    for (int s = 0; s < steps; ++s) {
      const int tl = 2 * s + kk;
      const float w = ws[tl];
      const float2 a = ys[abase + tl], y = ys[bbase + tl];
      const float ax = a.x * w, ay = a.y * w;
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, y.x, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, y.x, im, 0, 0, 0);
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, y.y, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(-ax, y.y, im, 0, 0, 0);
    }
  }
  const int npairs = wpe_pairs(E);
  float* __restrict__ dst = parts + (((int64_t)part * F + f) * npairs + wave) * 2048;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int row = (v & 3) + 8 * (v >> 2) + 4 * kk;
    dst[row * 32 + r] = re[v];
    dst[1024 + row * 32 + r] = im[v];
  }
}

// grid (F, utterances of the launch, slices), block 256: element (i, j), i >= j, j < D, of the lower triangle; i < D is
// R[i][j] and its mirror image, i >= D is conj(P[j][i - D]).
__global__ void __launch_bounds__(256) wpe_corr_reduce_kernel(const WpeTab tab, int C, int F, int K,
                                                              const float* __restrict__ parts, float2* __restrict__ R,
                                                              float2* __restrict__ P) {
  const int f = blockIdx.x, b = blockIdx.y;
  const int D = C * K, E = D + C, npairs = wpe_pairs(E);
  const int part0 = tab.rag.part_off[b], part1 = tab.rag.part_off[b + 1];
  float2* __restrict__ Rb = R + ((int64_t)b * F + f) * D * D;
  float2* __restrict__ Pb = P + ((int64_t)b * F + f) * D * C;
  for (int idx = blockIdx.z * 256 + threadIdx.x; idx < E * D; idx += 256 * gridDim.z) {
    const int i = idx / D, j = idx - i * D;
    if (j > i) continue;
    const int I = i >> 5, J = j >> 5;
    const int64_t o = (int64_t)(I * (I + 1) / 2 + J) * 2048 + (i & 31) * 32 + (j & 31);
    double sr = 0.0, si = 0.0;
    for (int part = part0; part < part1; ++part) {
      const float* __restrict__ src = parts + ((int64_t)part * F + f) * npairs * 2048 + o;
      sr += (double)src[0];
      si += (double)src[1024];
    }
    const float vr = (float)sr, vi = i == j ? 0.f : (float)si;
    if (i < D) {
      Rb[i * D + j] = make_float2(vr, vi);
      if (i != j) Rb[j * D + i] = make_float2(vr, -vi);
    } else {
      Pb[j * C + (i - D)] = make_float2(vr, -vi);
    }
  }
}

__device__ __forceinline__ int wpe_tri(int i, int k) { return i * (i + 1) / 2 + k; }

// grid (F, B), block 256.  bad[(b * slots + slot) * F + f] = 1 where the bin got G = 0 for a non-finite value.
__global__ void __launch_bounds__(256) wpe_solve_kernel(const float2* __restrict__ R, const float2* __restrict__ P, int C, int F,
                                                        int K, double diag_load, float2* __restrict__ G,
                                                        int32_t* __restrict__ bad, int slots, int slot) {
  __shared__ cd A[kWpeTri];
  __shared__ cd X[PK2_WPE_MAX_ORDER * PK2_WPE_MAX_CHANNELS];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int D = C * K, DC = D * C;
  const float2* __restrict__ Rb = R + ((int64_t)b * F + f) * D * D;
  const float2* __restrict__ Pb = P + ((int64_t)b * F + f) * DC;
  float2* __restrict__ Gb = G + ((int64_t)b * F + f) * DC;
  int nonfinite = 0;
  for (int idx = tid; idx < D * D; idx += 256) {
    const float2 v = Rb[idx];
    nonfinite |= !(isfinite(v.x) && isfinite(v.y));
    const int i = idx / D, k = idx - i * D;
    if (k <= i) A[wpe_tri(i, k)] = cd{(double)v.x, (double)v.y};
  }
  for (int idx = tid; idx < DC; idx += 256) {
    const float2 v = Pb[idx];
    nonfinite |= !(isfinite(v.x) && isfinite(v.y));
    X[idx] = cd{(double)v.x, (double)v.y};
  }
  int fail = __syncthreads_or(nonfinite);
  if (!fail) {
    double tr = 0.0;
    for (int d = 0; d < D; ++d) tr += A[wpe_tri(d, d)].x;
    const double load = diag_load * tr / D + 1e-10;
    __syncthreads();
    if (tid < D) {
      cd& a = A[wpe_tri(tid, tid)];
      a = cd{a.x + load, 0.0};
    }
    // right-looking Cholesky, R' = L L^H in place; two barriers per column.  The trailing update runs on a 16 x 16 grid of
    // threads over (row, column) of the lower triangle, so no index is divided.
    const int ty = tid >> 4, tx = tid & 15;
    for (int j = 0; j < D; ++j) {
      __syncthreads();                                          // the updates of column j are complete
      const double d = A[wpe_tri(j, j)].x;
      if (!(d > 0.0) || !isfinite(d)) { fail = 1; break; }      // the same value in every thread
      const double l = sqrt(d), inv = 1.0 / l;
      for (int i = j + 1 + tid; i < D; i += 256) {
        cd& a = A[wpe_tri(i, j)];
        a = cd{a.x * inv, a.y * inv};
      }
      __syncthreads();
      if (tid == 0) A[wpe_tri(j, j)] = cd{l, 0.0};          // nobody reads the pivot before the substitutions
      const int m = D - j - 1;
      for (int u = ty; u < m; u += 16) {
        const int i = j + 1 + u;
        const cd p = A[wpe_tri(i, j)];
        for (int v = tx; v <= u; v += 16) {
          const int k = j + 1 + v;
          const cd q = A[wpe_tri(k, j)];
          cd& a = A[wpe_tri(i, k)];                            // a -= p conj(q)
          a = cd{a.x - (p.x * q.x + p.y * q.y), i == k ? 0.0 : a.y - (p.y * q.x - p.x * q.y)};
        }
      }
    }
  }
  if (!fail) {
    // Column-oriented substitutions on an 8 (channels) x 32 (rows) grid of threads, one barrier per row: the thread that
    // finishes the next row's updates also divides it by its pivot.  Every element's updates stay in ascending (L Z = P)
    // and descending (L^H G = Z) order of i.
    const int sc = tid & 7, sr = tid >> 3;
    __syncthreads();
    if (tid < C) {
      const double inv = 1.0 / A[wpe_tri(0, 0)].x;
      cd& x = X[tid];
      x = cd{x.x * inv, x.y * inv};
    }
    for (int i = 0; i + 1 < D; ++i) {
      __syncthreads();
      if (sc < C) {
        const cd z = X[i * C + sc];
        for (int rr = i + 1 + sr; rr < D; rr += 32) {
          const cd l = A[wpe_tri(rr, i)];
          cd x = X[rr * C + sc];                               // x -= l z
          x = cd{x.x - (l.x * z.x - l.y * z.y), x.y - (l.x * z.y + l.y * z.x)};
          if (rr == i + 1) {
            const double inv = 1.0 / A[wpe_tri(rr, rr)].x;
            x = cd{x.x * inv, x.y * inv};
          }
          X[rr * C + sc] = x;
        }
      }
    }
    __syncthreads();
    if (tid < C) {
      const double inv = 1.0 / A[wpe_tri(D - 1, D - 1)].x;
      cd& x = X[(D - 1) * C + tid];
      x = cd{x.x * inv, x.y * inv};
    }
    for (int i = D - 1; i > 0; --i) {
      __syncthreads();
      if (sc < C) {
        const cd g = X[i * C + sc];
        for (int rr = i - 1 - sr; rr >= 0; rr -= 32) {
          const cd l = A[wpe_tri(i, rr)];
          cd x = X[rr * C + sc];                               // x -= conj(l) g
          x = cd{x.x - (l.x * g.x + l.y * g.y), x.y - (l.x * g.y - l.y * g.x)};
          if (rr == i - 1) {
            const double inv = 1.0 / A[wpe_tri(rr, rr)].x;
            x = cd{x.x * inv, x.y * inv};
          }
          X[rr * C + sc] = x;
        }
      }
    }
    __syncthreads();
    int inf = 0;
    for (int idx = tid; idx < DC; idx += 256) inf |= !(isfinite((float)X[idx].x) && isfinite((float)X[idx].y));
    fail = __syncthreads_or(inf);
  }
  for (int idx = tid; idx < DC; idx += 256)
    Gb[idx] = fail ? make_float2(0.f, 0.f) : make_float2((float)X[idx].x, (float)X[idx].y);
  if (tid == 0) bad[((int64_t)b * slots + slot) * F + f] = fail ? 1 : 0;
}

// grid (parts of 128 frames, ceil(F / 8)), block 256.  tab.out[b] and tab.power[b] may be null (not both).
template <int C>
__global__ void __launch_bounds__(256) wpe_filter_kernel(const WpeTab tab, int B, int F, int K, int delay,
                                                         const float2* __restrict__ G) {
  __shared__ float2 Gs[PK2_WPE_MAX_ORDER * PK2_WPE_MAX_CHANNELS * kWpeFB];
  __shared__ int live[kWpeFB];
  const int part = blockIdx.x;
  const int b = find_utt(tab.rag.part_off, B, part);
  const int tid = threadIdx.x, fl = tid & (kWpeFB - 1), tr = tid / kWpeFB;
  const int f0 = blockIdx.y * kWpeFB, f = f0 + fl;
  const int N = tab.rag.frames[b];
  const int DC = C * K * C;
  const int nbins = min(kWpeFB, F - f0);
  const float2* __restrict__ Gb = G + ((int64_t)b * F + f0) * DC;
  if (tid < kWpeFB) live[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < nbins * DC; idx += 256) {
    const int bl = idx / DC, e = idx - bl * DC;
    const float2 g = Gb[idx];
    Gs[e * kWpeFB + bl] = g;
    if (g.x != 0.f || g.y != 0.f) live[bl] = 1;        // every writer stores the same value
  }
  __syncthreads();
  const int tb = (part - tab.rag.part_off[b]) * kWpeFilterFrames + tr * kWpeTF;
  if (f >= F || tb >= N) return;
  const float2* __restrict__ Y = tab.spec[b];
  const int64_t NF = (int64_t)N * F;
  float2 x[C][kWpeTF], yw[C][kWpeTF];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < kWpeTF; ++j)
      x[c][j] = tb + j < N ? Y[c * NF + (int64_t)(tb + j) * F + f] : make_float2(0.f, 0.f);
  if (live[fl]) {
    for (int k = 0; k < K; ++k) {
      // yw[c][j] = Y[c, tb + j - delay - k]: a window that slides back by one frame per tap
      if (k == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int j = 0; j < kWpeTF; ++j) {
            const int t = tb + j - delay;
            yw[c][j] = (t >= 0 && t < N) ? Y[c * NF + (int64_t)t * F + f] : make_float2(0.f, 0.f);
          }
      } else {
        const int t = tb - delay - k;
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
          for (int j = kWpeTF - 1; j > 0; --j) yw[c][j] = yw[c][j - 1];
          yw[c][0] = t >= 0 ? Y[c * NF + (int64_t)t * F + f] : make_float2(0.f, 0.f);
        }
      }
      const float2* __restrict__ gk = Gs + (size_t)k * C * C * kWpeFB + fl;
#pragma unroll
      for (int ci = 0; ci < C; ++ci)
#pragma unroll
        for (int co = 0; co < C; ++co) {
          const float2 g = gk[(ci * C + co) * kWpeFB];
#pragma unroll
          for (int j = 0; j < kWpeTF; ++j) {
            // x -= conj(g) y
            const float2 y = yw[ci][j];
            x[co][j].x = fmaf(-g.x, y.x, x[co][j].x);
            x[co][j].x = fmaf(-g.y, y.y, x[co][j].x);
            x[co][j].y = fmaf(-g.x, y.y, x[co][j].y);
            x[co][j].y = fmaf(g.y, y.x, x[co][j].y);
          }
        }
    }
  }
  float2* __restrict__ out = tab.out[b];
  float* __restrict__ pw = tab.power[b];
  const float fc = (float)C;
#pragma unroll
  for (int j = 0; j < kWpeTF; ++j) {
    if (tb + j >= N) break;
    const int64_t o = (int64_t)(tb + j) * F + f;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (out) out[c * NF + o] = x[c][j];
      s = fmaf(x[c][j].x, x[c][j].x, s);
      s = fmaf(x[c][j].y, x[c][j].y, s);
    }
    if (pw) pw[o] = fmaxf(s / fc, 1e-10f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int wpe_check_shape(const char* who, int32_t B, int32_t C, int32_t F, int32_t K, int32_t delay) {
  if (int rc = check_shape(who, B, C, F)) return rc;
  PK2_REQUIRE(K >= 1 && (int64_t)C * K <= PK2_WPE_MAX_ORDER, "%s: %d taps on %d channels: the order C * taps must be in 1 to %d",
              who, K, C, PK2_WPE_MAX_ORDER);
  PK2_REQUIRE(delay >= 1 && delay <= PK2_WPE_MAX_DELAY, "%s: delay %d (1 to %d)", who, delay, PK2_WPE_MAX_DELAY);
  return PK2_OK;
}

// the workspace of one launch group (at most PK2_WPE_MAX_UTTS utterances)
struct WpeWork {
  float2* yt;
  float* wt;
  float* parts;
  float* power;
  float2 *R, *P, *G;
  int32_t* bad;
  size_t bytes;
};

static WpeWork wpe_carve(void* base, const int32_t* frames, int32_t nb, int32_t C, int32_t F, int32_t K) {
  int64_t total = 0, nparts = 0;
  for (int b = 0; b < nb; ++b) {
    total += frames[b];
    nparts += (frames[b] + kWpePart - 1) / kWpePart;
  }
  const int D = C * K;
  Carver cv(base);
  WpeWork w;
  w.yt = cv.take<float2>((size_t)total * C * F);
  w.wt = cv.take<float>((size_t)total * F);
  w.parts = cv.take<float>((size_t)nparts * F * wpe_pairs(D + C) * 2048);
  w.power = cv.take<float>((size_t)total * F);
  w.R = cv.take<float2>((size_t)nb * F * D * D);
  w.P = cv.take<float2>((size_t)nb * F * D * C);
  w.G = cv.take<float2>((size_t)nb * F * D * C);
  w.bad = cv.take<int32_t>((size_t)nb * PK2_WPE_MAX_ITERS * F);
  w.bytes = cv.bytes();
  return w;
}

static size_t wpe_solve_bytes(int32_t B, int32_t F) { return align_up((size_t)B * F * sizeof(int32_t), 256); }

// fills the table of one group; `gran` frames per part
static int wpe_fill(WpeTab& tab, const char* who, int32_t nb, int32_t C, int32_t F, const int32_t* frames, int gran,
                    int64_t* parts_out) {
  int64_t yoff = 0, woff = 0;
  for (int b = 0; b < nb; ++b) {
    tab.yoff[b] = yoff;
    tab.woff[b] = woff;
    yoff += (int64_t)frames[b] * C * F;
    woff += (int64_t)frames[b] * F;
  }
  return fill_ragged(who, tab.rag, frames, 0, nb, gran, parts_out);
}

static int wpe_launch_power(WpeTab& tab, int nb, int C, int F, const int32_t* frames, hipStream_t stream) {
  int64_t parts;
  if (int rc = wpe_fill(tab, "wpe_power", nb, C, F, frames, 32, &parts)) return rc;
  hipLaunchKernelGGL(wpe_power_kernel, dim3((unsigned)parts, (unsigned)((F + 63) / 64)), dim3(64), 0, stream, tab, nb, C, F);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

// tab.spec / tab.weight -> wk.yt / wk.wt
static int wpe_launch_transpose(WpeTab& tab, int nb, int C, int F, const int32_t* frames, bool do_spec, bool do_weight,
                                const WpeWork& wk, hipStream_t stream) {
  int64_t parts;
  if (int rc = wpe_fill(tab, "wpe_corr", nb, C, F, frames, 32, &parts)) return rc;
  const unsigned planes = (do_spec ? C : 0) + (do_weight ? 1 : 0);
  hipLaunchKernelGGL(wpe_transpose_kernel, dim3((unsigned)parts, (unsigned)((F + 31) / 32), planes), dim3(256), 0, stream, tab,
                     nb, C, F, do_spec ? 1 : 0, wk.yt, wk.wt);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

// wk.yt, wk.wt -> R, P (of this group)
static int wpe_launch_corr(WpeTab& tab, int nb, int C, int F, int K, int delay, const int32_t* frames, const WpeWork& wk,
                           float2* R, float2* P, hipStream_t stream) {
  int64_t parts;
  if (int rc = wpe_fill(tab, "wpe_corr", nb, C, F, frames, kWpePart, &parts)) return rc;
  const int E = C * K + C;
  hipLaunchKernelGGL(wpe_corr_kernel, dim3((unsigned)parts, (unsigned)F), dim3(64 * wpe_pairs(E)), 0, stream, tab, nb, C, F, K,
                     delay, wk.yt, wk.wt, wk.parts);
  PK2_LAUNCH_CHECK();
  const unsigned slices = (unsigned)std::min(8, (E * C * K + 255) / 256);
  hipLaunchKernelGGL(wpe_corr_reduce_kernel, dim3((unsigned)F, (unsigned)nb, slices), dim3(256), 0, stream, tab, C, F, K,
                     wk.parts, R, P);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

static int wpe_launch_filter(WpeTab& tab, int nb, int C, int F, int K, int delay, const int32_t* frames, const float2* G,
                             hipStream_t stream) {
  int64_t parts;
  if (int rc = wpe_fill(tab, "wpe_filter", nb, C, F, frames, kWpeFilterFrames, &parts)) return rc;
  const dim3 grid((unsigned)parts, (unsigned)((F + kWpeFB - 1) / kWpeFB)), block(256);
  dispatch_channels(C, [&](auto c) {
    hipLaunchKernelGGL(wpe_filter_kernel<decltype(c)::value>, grid, block, 0, stream, tab, nb, F, K, delay, G);
  });
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

static bool wpe_shape_ok(int32_t B, int32_t C, int32_t F, int32_t K, int32_t delay) {
  return B >= 1 && C >= 1 && C <= PK2_WPE_MAX_CHANNELS && F >= 1 && F <= 4097 && K >= 1 &&
         (int64_t)C * K <= PK2_WPE_MAX_ORDER && delay >= 1 && delay <= PK2_WPE_MAX_DELAY;
}

static size_t wpe_total_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t K) {
  size_t need = 0;
  for (int b0 = 0; b0 < B; b0 += PK2_WPE_MAX_UTTS)
    need += wpe_carve(nullptr, frames + b0, std::min<int>(PK2_WPE_MAX_UTTS, B - b0), C, F, K).bytes;
  return need;
}

}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_wpe_workspace_bytes(const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t taps, int32_t delay) {
  if (!frames || !wpe_shape_ok(B, C, F, taps, delay)) return 0;
  for (int b = 0; b < B; ++b)
    if (frames[b] < 1 || frames[b] > (1 << 24)) return 0;
  return wpe_total_bytes(frames, B, C, F, taps);
}

extern "C" int pk2_wpe_power(const float* const* spec, const int32_t* frames, int32_t B, int32_t C, int32_t F,
                             float* const* power, void* stream_) {
  if (int rc = wpe_check_shape("wpe_power", B, C, F, 1, 1)) return rc;
  if (int rc = check_frames("wpe_power", frames, B)) return rc;
  if (int rc = check_table("wpe_power", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("wpe_power", "the power", power, B)) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for (int b0 = 0; b0 < B; b0 += PK2_WPE_MAX_UTTS) {
    const int nb = std::min<int>(PK2_WPE_MAX_UTTS, B - b0);
    WpeTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      tab.power[b] = power[b0 + b];
    }
    if (int rc = wpe_launch_power(tab, nb, C, F, frames + b0, stream)) return rc;
  }
  return PK2_OK;
}

extern "C" int pk2_wpe_corr(const float* const* spec, const float* const* weight, const int32_t* frames, int32_t B, int32_t C,
                            int32_t F, int32_t taps, int32_t delay, void* work, size_t work_bytes, float* R, float* P,
                            void* stream_) {
  if (int rc = wpe_check_shape("wpe_corr", B, C, F, taps, delay)) return rc;
  if (int rc = check_frames("wpe_corr", frames, B)) return rc;
  if (int rc = check_table("wpe_corr", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("wpe_corr", "the weight", weight, B)) return rc;
  PK2_REQUIRE(work && R && P, "wpe_corr: null pointer");
  const size_t need = wpe_total_bytes(frames, B, C, F, taps);
  PK2_REQUIRE(work_bytes >= need, "wpe_corr: workspace of %zu bytes, %zu needed", work_bytes, need);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int D = C * taps;
  char* wbase = static_cast<char*>(work);
  for (int b0 = 0; b0 < B; b0 += PK2_WPE_MAX_UTTS) {
    const int nb = std::min<int>(PK2_WPE_MAX_UTTS, B - b0);
    const WpeWork wk = wpe_carve(wbase, frames + b0, nb, C, F, taps);
    wbase += wk.bytes;
    WpeTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      tab.weight[b] = weight[b0 + b];
    }
    if (int rc = wpe_launch_transpose(tab, nb, C, F, frames + b0, true, true, wk, stream)) return rc;
    if (int rc = wpe_launch_corr(tab, nb, C, F, taps, delay, frames + b0, wk,
                                 reinterpret_cast<float2*>(R) + (int64_t)b0 * F * D * D,
                                 reinterpret_cast<float2*>(P) + (int64_t)b0 * F * D * C, stream))
      return rc;
  }
  return PK2_OK;
}

extern "C" int pk2_wpe_solve(const float* R, const float* P, int32_t B, int32_t C, int32_t F, int32_t taps, double diag_load,
                             void* work, size_t work_bytes, float* G, int32_t* nonfinite, void* stream_) {
  if (int rc = wpe_check_shape("wpe_solve", B, C, F, taps, 1)) return rc;
  PK2_REQUIRE(diag_load >= 0.0 && diag_load < 1e30, "wpe_solve: diag_load %g must be finite and >= 0", diag_load);
  PK2_REQUIRE(R && P && work && G && nonfinite, "wpe_solve: null pointer");
  PK2_REQUIRE(work_bytes >= wpe_solve_bytes(B, F), "wpe_solve: workspace of %zu bytes, %zu needed", work_bytes,
              wpe_solve_bytes(B, F));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int32_t* bad = static_cast<int32_t*>(work);
  hipLaunchKernelGGL(wpe_solve_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, stream, reinterpret_cast<const float2*>(R),
                     reinterpret_cast<const float2*>(P), C, F, taps, diag_load, reinterpret_cast<float2*>(G), bad, 1, 0);
  PK2_LAUNCH_CHECK();
  hipLaunchKernelGGL(any_flag_kernel<256>, dim3((unsigned)B), dim3(256), 0, stream, bad, F, nonfinite);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_wpe_filter(const float* const* spec, const float* G, const int32_t* frames, int32_t B, int32_t C, int32_t F,
                              int32_t taps, int32_t delay, float* const* out, float* const* power_out, void* stream_) {
  if (int rc = wpe_check_shape("wpe_filter", B, C, F, taps, delay)) return rc;
  if (int rc = check_frames("wpe_filter", frames, B)) return rc;
  if (int rc = check_table("wpe_filter", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("wpe_filter", "the output", out, B)) return rc;
  if (power_out)
    if (int rc = check_table("wpe_filter", "the power", power_out, B)) return rc;
  PK2_REQUIRE(G, "wpe_filter: G is null");
  for (int b = 0; b < B; ++b) PK2_REQUIRE(out[b] != spec[b], "wpe_filter: the output of utterance %d is its spectrum", b);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int D = C * taps;
  for (int b0 = 0; b0 < B; b0 += PK2_WPE_MAX_UTTS) {
    const int nb = std::min<int>(PK2_WPE_MAX_UTTS, B - b0);
    WpeTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      tab.out[b] = reinterpret_cast<float2*>(out[b0 + b]);
      tab.power[b] = power_out ? power_out[b0 + b] : nullptr;
    }
    if (int rc = wpe_launch_filter(tab, nb, C, F, taps, delay, frames + b0,
                                   reinterpret_cast<const float2*>(G) + (int64_t)b0 * F * D * C, stream))
      return rc;
  }
  return PK2_OK;
}

extern "C" int pk2_wpe(const float* const* spec, const int32_t* frames, int32_t B, int32_t C, int32_t F, int32_t taps,
                       int32_t delay, int32_t iters, double diag_load, void* work, size_t work_bytes, float* const* out,
                       int32_t* nonfinite, void* stream_) {
  if (int rc = wpe_check_shape("wpe", B, C, F, taps, delay)) return rc;
  PK2_REQUIRE(iters >= 1 && iters <= PK2_WPE_MAX_ITERS, "wpe: %d iterations (1 to %d)", iters, PK2_WPE_MAX_ITERS);
  PK2_REQUIRE(diag_load >= 0.0 && diag_load < 1e30, "wpe: diag_load %g must be finite and >= 0", diag_load);
  if (int rc = check_frames("wpe", frames, B)) return rc;
  if (int rc = check_table("wpe", "the spectrum", spec, B)) return rc;
  if (int rc = check_table("wpe", "the output", out, B)) return rc;
  PK2_REQUIRE(work && nonfinite, "wpe: null pointer");
  for (int b = 0; b < B; ++b) PK2_REQUIRE(out[b] != spec[b], "wpe: the output of utterance %d is its spectrum", b);
  const size_t need = wpe_total_bytes(frames, B, C, F, taps);
  PK2_REQUIRE(work_bytes >= need, "wpe: workspace of %zu bytes, %zu needed", work_bytes, need);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* wbase = static_cast<char*>(work);
  for (int b0 = 0; b0 < B; b0 += PK2_WPE_MAX_UTTS) {
    const int nb = std::min<int>(PK2_WPE_MAX_UTTS, B - b0);
    const int32_t* fr = frames + b0;
    const WpeWork wk = wpe_carve(wbase, fr, nb, C, F, taps);
    wbase += wk.bytes;
    WpeTab tab;
    memset(&tab, 0, sizeof(tab));
    int64_t poff = 0;
    float* pw[PK2_WPE_MAX_UTTS];
    for (int b = 0; b < nb; ++b) {
      tab.spec[b] = reinterpret_cast<const float2*>(spec[b0 + b]);
      pw[b] = wk.power + poff;
      poff += (int64_t)fr[b] * F;
      tab.power[b] = pw[b];
      tab.weight[b] = pw[b];
    }
    if (int rc = wpe_launch_power(tab, nb, C, F, fr, stream)) return rc;
    for (int it = 0; it < iters; ++it) {
      const bool last = it + 1 == iters;
      if (int rc = wpe_launch_transpose(tab, nb, C, F, fr, it == 0, true, wk, stream)) return rc;
      if (int rc = wpe_launch_corr(tab, nb, C, F, taps, delay, fr, wk, wk.R, wk.P, stream)) return rc;
      hipLaunchKernelGGL(wpe_solve_kernel, dim3((unsigned)F, (unsigned)nb), dim3(256), 0, stream, wk.R, wk.P, C, F, taps,
                         diag_load, wk.G, wk.bad, iters, it);
      PK2_LAUNCH_CHECK();
      for (int b = 0; b < nb; ++b) {
        tab.out[b] = last ? reinterpret_cast<float2*>(out[b0 + b]) : nullptr;
        tab.power[b] = last ? nullptr : pw[b];
      }
      if (int rc = wpe_launch_filter(tab, nb, C, F, taps, delay, fr, wk.G, stream)) return rc;
    }
    hipLaunchKernelGGL(any_flag_kernel<256>, dim3((unsigned)nb), dim3(256), 0, stream, wk.bad, iters * F, nonfinite + b0);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}
