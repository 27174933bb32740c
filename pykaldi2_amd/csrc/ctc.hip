// Connectionist temporal classification on gfx950: loss and gradient of a minibatch from unnormalised logits, fused
// (DESIGN.md 7.19).  With y_t = softmax(x[t, .]) and the extended sequence blank, l_1, blank, .., l_L, blank (S = 2 L + 1):
//
//   alpha_0(0) = y_0(blank), alpha_0(1) = y_0(l_1)     alpha_t(s) = y_t(ext_s) [alpha_{t-1}(s) + alpha_{t-1}(s-1) + skip_s alpha_{t-1}(s-2)]
//   p = alpha_{T-1}(S-1) + alpha_{T-1}(S-2)            loss = -log p
//   grad[t, k] = w ( y_t(k) - sum_{s: ext_s = k} P(state s at frame t) )
//
// The trellis is regular, so there are no arc lists.  States are held as PAIRS (blank_i, label_i), i = 0..L (the last pair
// has a blank only); skip_i = 1 iff i >= 1 and l_{i+1} != l_i (the label of pair i may be entered from the label of pair i-1):
//
//   alpha:  blank_i(t) = e_t(0)   (blank_i + label_{i-1})(t-1)
//           label_i(t) = e_t(i+1) (label_i + blank_i + skip_i label_{i-1})(t-1)
//   beta (WITHOUT the emission of its own frame, so that the occupancy is alpha * beta with no division by y):
//           hb_i(t) = ub_i + ul_i,   hl_i(t) = ul_i + c_{i+1}    with, of frame t+1,  ub_i = hb_i e(0), ul_i = hl_i e(i+1),
//           c_i = ub_i + skip_i ul_i  (what pair i hands to the label on its left: one value per pair, as in the alpha chain)
//
// Three launches on one stream, none waits on another workgroup, nothing is read back:
//   ctc_rows    a wave per frame: one pass over the P logits (vector loads) for m_t = max and 1 / sum exp(x - m_t), then the
//               compact emission row e[t, 0] = y_t(blank), e[t, j] = y_t(l_j): L + 1 floats per frame.
//   ctc_chains  two workgroups per utterance, alpha from frame 0 up and beta from frame T-1 down, in probability space with
//               one scale per frame applied lazily (the csrc/chain_num_graph.hip scheme).  A lane owns K = ceil((L+1) / 512)
//               consecutive pairs in registers; the one neighbour value per frame comes by a cross-lane shift, across a wave
//               boundary through one LDS word per wave.  LDS holds only that word and the wave partial sums of the frame, both
//               double-buffered: one barrier per frame.  The emissions of the next frame are loaded ahead of the barrier.
//               Three things keep the two chains' product, where the posterior lives, inside the number format (DESIGN.md
//               7.19): a chain keeps only the states its partner can meet (alpha: those that can still reach the end, beta:
//               those reachable from the start); state s is carried as alpha(s) theta^s / beta(s) theta^-s, i.e. the moves
//               stay / next / skip weigh 1, theta, theta^2 with theta set by the advance per frame the utterance needs
//               (ctc_tilt); and the chains, their rows in the workspace and the frame totals are float64 (emissions stay f32).
//   ctc_grad    a workgroup per frame: w y_t(k) on all P columns; occupancies alpha * beta normalised by the frame's own total
//               (the two chains' scales cancel); after a barrier ONE thread per distinct label adds its states in the sorted
//               order of the packed descriptor and rewrites that column: no atomics, the call is bit-reproducible, and an
//               utterance's result does not depend on its neighbours (K and every sum depend on its own L only).
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = (PK2_CTC_MAX_LABELS + 1 + kThreads - 1) / kThreads;      // 8 pairs per lane at the length limit
constexpr int kGradThreads = 256;

// Packed descriptor (int32 words, made by pykaldi2_amd/ctc.py): N of these, then per utterance its labels [L], the label
// positions 0..L-1 sorted by (label, position) [L] and the labels in that order [L].
struct CtcDesc {
  int32_t T, L, status, lab, ord;
  float w;
  int32_t pad[2];
};
static_assert(sizeof(CtcDesc) == 32, "CtcDesc is 8 words");

// Workspace of one utterance with status 0, in floats from its base (every array on a 64-word boundary).
struct CtcLayout {
  size_t e, mz, al, be, zs, flag, words;
};
__host__ __device__ inline size_t ctc_up(size_t x) { return (x + 63) / 64 * 64; }
__host__ __device__ inline CtcLayout ctc_layout(size_t T, size_t L) {
  CtcLayout l;
  size_t o = 0;
  l.e = o; o += ctc_up(T * (L + 1));          // f32 [T][L+1]      y_t(blank), y_t(l_1), .., y_t(l_L)
  l.mz = o; o += ctc_up(2 * T);               // f32 [T][2]        m_t, 1 / sum exp(x - m_t)
  l.al = o; o += ctc_up(4 * T * (L + 1));     // f64 [T][L+1][2]   stored alpha (blank_i, label_i)
  l.be = o; o += ctc_up(4 * T * (L + 1));     // f64 [T][L+1][2]   stored beta
  l.zs = o; o += ctc_up(2 * T);               // f64 [T]           sums of the stored alpha rows
  l.flag = o; o += 64;                        // i32 [2]           1: the beta / the alpha chain met a zero or non-finite scale
  l.words = o;
  return l;
}
__device__ inline size_t ctc_base(const CtcDesc* desc, int n) {
  size_t o = 0;
  for (int m = 0; m < n; ++m)
    if (desc[m].status == 0) o += ctc_layout(desc[m].T, desc[m].L).words;
  return o;
}

// ---- ctc_rows: grid (blocks, N), a wave per frame.
__global__ __launch_bounds__(256) void ctc_rows(const int32_t* __restrict__ pk, const float* __restrict__ x, int64_t seq_stride,
                                                int64_t frame_stride, int32_t P, int32_t blank, float* __restrict__ ws) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const CtcDesc* desc = reinterpret_cast<const CtcDesc*>(pk);
  const CtcDesc d = desc[n];
  if (d.status != 0) return;
  const int T = d.T, L = d.L;
  const CtcLayout l = ctc_layout(T, L);
  float* base = ws + ctc_base(desc, n);
  const int32_t* lab = pk + d.lab;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (int t = wave; t < T; t += nwaves) {
    const float* row = x + (int64_t)n * seq_stride + (int64_t)t * frame_stride;
    // the row as [head scalars][16-byte aligned float4s][tail scalars]; the scalars are at most 6, one lane each
    const int head = min(P, (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) >> 2));
    const int nvec = (P - head) >> 2, tail0 = head + 4 * nvec;
    float m = -INFINITY, s = 0.f;
    for (int v = lane; v < nvec; v += 64) {
      const float4 q = *reinterpret_cast<const float4*>(row + head + 4 * v);
      const float mn = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
      const float part = (__expf(q.x - mn) + __expf(q.y - mn)) + (__expf(q.z - mn) + __expf(q.w - mn));
      s = s * __expf(m - mn) + part;
      m = mn;
    }
    if (lane < head + P - tail0) {
      const float v = row[lane < head ? lane : tail0 + lane - head];
      const float mn = fmaxf(m, v);
      s = s * __expf(m - mn) + __expf(v - mn);
      m = mn;
    }
    const float M = pk2::wave_max(m);
    s = s * __expf(m - M);                      // a lane without an element has s = 0, m = -inf: 0 * 0
    const float inv = 1.f / pk2::wave_sum(s);
    float* erow = base + l.e + (size_t)t * (L + 1);
    for (int j = lane; j <= L; j += 64) erow[j] = __expf(row[j ? lab[j - 1] : blank] - M) * inv;
    if (lane == 0) {
      (base + l.mz)[2 * (size_t)t] = M;
      (base + l.mz)[2 * (size_t)t + 1] = inv;
    }
  }
}

// The tilt of utterance (T, L): theta > 0 with (theta + 2 theta^2) / (1 + theta + theta^2) = 2 L / (T - 1), the mean advance per
// frame that a path needs.  State s is carried as alpha(s) theta^s (beta: theta^-s), i.e. the three moves stay / next / skip
// weigh 1, theta, theta^2 in both chains and the product alpha * beta is unchanged.
__device__ inline double ctc_tilt(int T, int L) {
  if (L == 0 || T < 2) return 1.0;
  const double r = fmin(2.0 * L / (T - 1.0), 1.999), a = r - 2.0, b = r - 1.0;
  const double th = (-b - sqrt(b * b - 4.0 * a * r)) / (2.0 * a);
  return fmin(fmax(th, 1.0 / 4096), 4096.0);
}

// ---- ctc_chains: grid (2, N).  blockIdx.x = 0: alpha, loss and status; 1: beta.
__global__ __launch_bounds__(kThreads) void ctc_chains(const int32_t* __restrict__ pk, float* __restrict__ ws, double* __restrict__ loss,
                                                       int32_t* __restrict__ status) {
  __shared__ double wsum[2][kWaves];     // wave partial sums of the frame
  __shared__ double bnd[2][kWaves];      // the value a wave hands to its neighbour wave
  __shared__ double dred[kWaves];
  const int n = blockIdx.y, tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const bool fwd = blockIdx.x == 0;
  const CtcDesc* desc = reinterpret_cast<const CtcDesc*>(pk);
  const CtcDesc d = desc[n];
  if (d.status != 0) {
    if (fwd && tx == 0) { loss[n] = 0.0; status[n] = d.status; }
    return;
  }
  const int T = d.T, L = d.L, NP = L + 1;
  const int K = (NP + kThreads - 1) / kThreads;      // pairs per lane: of this utterance, whatever its neighbours need
  const int i0 = tx * K;
  const CtcLayout l = ctc_layout(T, L);
  float* base = ws + ctc_base(desc, n);
  const float* e = base + l.e;
  const int32_t* lab = pk + d.lab;
  const double th = ctc_tilt(T, L), th2 = th * th;
  uint32_t valid = 0, skip = 0;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    const int i = i0 + k;
    if (k < K && i < NP) {
      valid |= 1u << k;
      if (i >= 1 && i < L && lab[i] != lab[i - 1]) skip |= 1u << k;
    }
  }
  auto frame_sum = [&](int t) {
    double z = wsum[t & 1][0];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) z += wsum[t & 1][q];
    return z;
  };
  auto publish = [&](int t, double v) {
    v = pk2::wave_sum_d(v);
    if (lane == 0) wsum[t & 1][wave] = v;
  };
  float el[kMaxK], en[kMaxK], e0, e0n;      // emissions of this frame / of the next one
  auto load = [&](int t) {
    const float* erow = e + (size_t)t * NP;
    e0n = erow[0];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) en[k] = (k < K && i0 + k < L) ? erow[i0 + k + 1] : 0.f;
  };
  if (fwd) {
    double2* a2 = reinterpret_cast<double2*>(base + l.al);
    double* zs = reinterpret_cast<double*>(base + l.zs);
    double vb[kMaxK], vl[kMaxK], last = 0.0;      // last: the label of the lane's last pair, what the lane on the right needs
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) vb[k] = vl[k] = 0.0;
    load(0);
    for (int t = 0; t < T; ++t) {
      e0 = e0n;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) el[k] = en[k];
      if (t + 1 < T) load(t + 1);
      double2* arow = a2 + (size_t)t * NP;
      double mysum = 0.0;
      if (t == 0) {
        if (tx == 0) { vb[0] = e0; vl[0] = th * el[0]; }
      } else {
        const double z = frame_sum(t - 1);
        const double inv = 1.0 / z;
        if (tx == 0) zs[t - 1] = z;
        double carry = __shfl_up(last, 1, 64);
        if (lane == 0) carry = wave > 0 ? bnd[(t - 1) & 1][wave - 1] : 0.0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
          if (k < K) {
            const double ob = vb[k], ol = vl[k];
            const double eb = ((valid >> k) & 1) ? e0 * inv : 0.0;
            const double nb = eb * (ob + th * carry);
            const double nl = (el[k] * inv) * ((ol + th * ob) + (((skip >> k) & 1) ? th2 * carry : 0.0));
            vb[k] = nb;
            vl[k] = nl;
            carry = ol;
          }
      }
      // only the states that can still reach the end in the frames left take part (state 2 i + 1 >= S - 2 (T - t)): the
      // frame's scale is then that of the paths that count, not of the many cheap ones that cannot finish
      const int dead = L - (T - t);
#pragma unroll
      for (int k = 0; k < kMaxK; ++k)
        if (k < K) {
          if (i0 + k <= dead) vb[k] = 0.0;
          if (i0 + k < dead) vl[k] = 0.0;
          if ((valid >> k) & 1) arow[i0 + k] = make_double2(vb[k], vl[k]);
          mysum += vb[k] + vl[k];
          if (k == K - 1) last = vl[k];
        }
      publish(t, mysum);
      if (lane == 63) bnd[t & 1][wave] = last;
      __syncthreads();
    }
    // log p = sum_{t < T-1} log z_t + log(the two final states of the last stored row) - 2 L log theta
    pk2::block_sync_global();
    double acc = 0.0;
    for (int t = tx; t < T - 1; t += kThreads) acc += log(zs[t]);
    acc = pk2::wave_sum_d(acc);
    if (lane == 0) dred[wave] = acc;
    __syncthreads();
    if (tx == 0) {
      const double* lrow = reinterpret_cast<const double*>(base + l.al) + (size_t)(T - 1) * 2 * NP;
      const double fin = lrow[2 * L] + (L > 0 ? th * lrow[2 * L - 1] : 0.0);
      double tot = log(fin) - 2.0 * L * log(th);
      for (int q = 0; q < kWaves; ++q) tot += dred[q];
      const bool ok = tot == tot && tot > -INFINITY && tot < INFINITY;      // a scale that was 0, inf or NaN shows here
      loss[n] = ok ? -tot : 0.0;
      status[n] = ok ? PK2_CTC_OK : PK2_CTC_NUMERIC;
      reinterpret_cast<int32_t*>(base + l.flag)[1] = ok ? 0 : 1;
    }
  } else {
    double2* h2 = reinterpret_cast<double2*>(base + l.be);
    double ub[kMaxK], ul[kMaxK], c[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) ub[k] = ul[k] = c[k] = 0.0;
    bool bad = false;
    load(T - 1);
    for (int t = T - 1; t >= 0; --t) {
      e0 = e0n;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) el[k] = en[k];
      if (t > 0) load(t - 1);
      double2* hrow = h2 + (size_t)t * NP;
      double inv = 0.0, right = 0.0;
      if (t < T - 1) {
        const double z = frame_sum(t + 1);
        bad = bad || !(z > 0.0 && z < INFINITY);
        inv = 1.0 / z;
        right = __shfl_down(c[0], 1, 64);
        if (lane == 63) right = wave + 1 < kWaves ? bnd[(t + 1) & 1][wave + 1] : 0.0;
      }
      double mysum = 0.0;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k)
        if (k < K) {
          const int i = i0 + k;
          double hb, hl;
          if (t == T - 1) {
            hb = i == L ? 1.0 : 0.0;
            hl = i == L - 1 ? th : 0.0;
          } else {
            const double cr = k + 1 < K ? c[(k + 1) % kMaxK] : right;      // (the pair on the right: own, or the next lane's first)
            hb = (ub[k] + th * ul[k]) * inv;
            hl = (ul[k] + th * cr) * inv;
          }
          if (i > t) hb = hl = 0.0;      // the mirror of the alpha chain's rule: states that no path has reached by frame t
          if ((valid >> k) & 1) hrow[i] = make_double2(hb, hl);
          ub[k] = ((valid >> k) & 1) ? hb * e0 : 0.0;
          ul[k] = hl * el[k];
          c[k] = ub[k] + (((skip >> k) & 1) ? th * ul[k] : 0.0);
          mysum += hb + hl;
        }
      publish(t, mysum);
      if (lane == 0) bnd[t & 1][wave] = c[0];
      __syncthreads();
    }
    if (tx == 0) reinterpret_cast<int32_t*>(base + l.flag)[0] = bad ? 1 : 0;
  }
}

// ---- ctc_grad: grid (Tpad, N), Lmax + 1 floats of LDS.  Writes every row of grad: zeros past the utterance's frames and
// for an utterance whose status is not 0.
__global__ __launch_bounds__(kGradThreads) void ctc_grad(const int32_t* __restrict__ pk, const float* __restrict__ x, int64_t seq_stride,
                                                         int64_t frame_stride, int32_t P, int32_t blank, const float* __restrict__ ws,
                                                         float* __restrict__ grad, int64_t gss, int64_t gfs, double* __restrict__ loss,
                                                         int32_t* __restrict__ status) {
  extern __shared__ __align__(16) float q[];      // occupancy of state s at this frame
  __shared__ double red[2][kGradThreads / 64];
  const int n = blockIdx.y, t = blockIdx.x, tx = threadIdx.x;
  const CtcDesc* desc = reinterpret_cast<const CtcDesc*>(pk);
  const CtcDesc d = desc[n];
  float* grow = grad + (int64_t)n * gss + (int64_t)t * gfs;
  const float* base = nullptr;
  CtcLayout l = {};
  bool live = d.status == 0;
  if (live) {
    base = ws + ctc_base(desc, n);
    l = ctc_layout(d.T, d.L);
    const int32_t* flag = reinterpret_cast<const int32_t*>(base + l.flag);
    const bool beta_bad = flag[0] != 0;
    if (beta_bad && t == 0 && tx == 0) { status[n] = PK2_CTC_NUMERIC; loss[n] = 0.0; }
    live = !beta_bad && flag[1] == 0 && t < d.T;
  }
  if (!live) {
    for (int k = tx; k < P; k += kGradThreads) grow[k] = 0.f;
    return;
  }
  const int L = d.L, NP = L + 1;
  const double2* arow = reinterpret_cast<const double2*>(base + l.al) + (size_t)t * NP;
  const double2* hrow = reinterpret_cast<const double2*>(base + l.be) + (size_t)t * NP;
  double sb = 0.0, sl = 0.0;
  for (int i = tx; i < NP; i += kGradThreads) {
    const double2 a = arow[i], h = hrow[i];
    sb += a.x * h.x;
    sl += a.y * h.y;
  }
  sb = pk2::wave_sum_d(sb);
  sl = pk2::wave_sum_d(sl);
  if ((tx & 63) == 0) { red[0][tx >> 6] = sb; red[1][tx >> 6] = sl; }
  const float* row = x + (int64_t)n * seq_stride + (int64_t)t * frame_stride;
  const float M = (base + l.mz)[2 * (size_t)t], inv = (base + l.mz)[2 * (size_t)t + 1], w = d.w;
  for (int k = tx; k < P; k += kGradThreads) grow[k] = w * (__expf(row[k] - M) * inv);
  __syncthreads();
  const double blanks = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  const double tot = blanks + ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
  if (!(tot > 1e-290 && tot < INFINITY)) {      // the products of two normalised rows left the number format
    for (int k = tx; k < P; k += kGradThreads) grow[k] = 0.f;
    if (tx == 0) status[n] = PK2_CTC_NUMERIC;
    return;
  }
  const double itot = 1.0 / tot;
  for (int i = tx; i < L; i += kGradThreads) q[i] = (float)(arow[i].y * hrow[i].y * itot);      // label states only
  if (tx == 0) grow[blank] = w * (__expf(row[blank] - M) * inv) - w * (float)(blanks * itot);
  __syncthreads();
  const int32_t* ord = pk + d.ord;
  const int32_t* slab = ord + L;
  for (int r = tx; r < L; r += kGradThreads) {
    const int32_t p = slab[r];
    if (r > 0 && slab[r - 1] == p) continue;      // the first slot of a label adds the whole group, in sorted order
    float acc = 0.f;
    for (int k = r; k < L && slab[k] == p; ++k) acc += q[ord[k]];
    grow[p] = w * (__expf(row[p] - M) * inv) - w * acc;
  }
}

// Host-side check of the packed descriptor: everything a kernel indexes with is verified here, against the host copy.
int ctc_check(const int32_t* pk, int64_t words, int32_t N, int32_t Tpad, int32_t P, int32_t blank, size_t* ws_words, int32_t* Tmax,
              int32_t* Lmax) {
  PK2_REQUIRE(pk && N >= 1 && words >= (int64_t)N * 8, "ctc: descriptor of %lld words for %d utterances", (long long)words, N);
  const CtcDesc* desc = reinterpret_cast<const CtcDesc*>(pk);
  *ws_words = 0; *Tmax = 0; *Lmax = 0;
  for (int32_t n = 0; n < N; ++n) {
    const CtcDesc& d = desc[n];
    PK2_REQUIRE(d.T >= 0 && d.T <= Tpad, "ctc: utterance %d has %d frames, the tensor %d", n, d.T, Tpad);
    if (d.L < 0 || d.L > PK2_CTC_MAX_LABELS) {
      pk2::set_error("ctc: utterance %d has %d labels (limit %d)", n, d.L, PK2_CTC_MAX_LABELS);
      return PK2_ERR_LIMIT;
    }
    PK2_REQUIRE(d.lab >= N * 8 && d.ord >= N * 8 && (int64_t)d.lab + d.L <= words && (int64_t)d.ord + 2 * (int64_t)d.L <= words,
                "ctc: utterance %d: label arrays outside the descriptor", n);
    const int32_t* lab = pk + d.lab;
    const int32_t* ord = pk + d.ord;
    const int32_t* slab = ord + d.L;
    int32_t repeats = 0;
    for (int32_t i = 0; i < d.L; ++i) {
      PK2_REQUIRE(lab[i] >= 0 && lab[i] < P && lab[i] != blank, "ctc: utterance %d: label %d at %d (%d columns, blank %d)", n, lab[i], i,
                  P, blank);
      if (i > 0 && lab[i] == lab[i - 1]) ++repeats;
      PK2_REQUIRE(ord[i] >= 0 && ord[i] < d.L && lab[ord[i]] == slab[i] &&
                      (i == 0 || slab[i - 1] < slab[i] || (slab[i - 1] == slab[i] && ord[i - 1] < ord[i])),
                  "ctc: utterance %d: label positions not sorted by (label, position) at %d", n, i);
    }
    const int32_t want = d.T >= 1 && d.T >= d.L + repeats ? PK2_CTC_OK : PK2_CTC_NO_PATH;
    PK2_REQUIRE(d.status == want, "ctc: utterance %d: status %d, %d frames for %d labels with %d repeats", n, d.status, d.T, d.L, repeats);
    if (d.status == 0) {
      *ws_words += ctc_layout(d.T, d.L).words;
      *Tmax = std::max(*Tmax, d.T);
      *Lmax = std::max(*Lmax, d.L);
    }
  }
  return PK2_OK;
}

}  // namespace

extern "C" {

size_t pk2_ctc_workspace_bytes(const int32_t* packed, int32_t num_utts) {
  if (!packed || num_utts < 1) return 0;
  const CtcDesc* desc = reinterpret_cast<const CtcDesc*>(packed);
  size_t words = 0;
  for (int32_t n = 0; n < num_utts; ++n)
    if (desc[n].status == 0 && desc[n].T >= 1 && desc[n].L >= 0 && desc[n].L <= PK2_CTC_MAX_LABELS)
      words += ctc_layout(desc[n].T, desc[n].L).words;
  return pk2::align_up(words * 4 + 256, 256);
}

int pk2_ctc_loss_and_grad(const int32_t* packed, const int32_t* packed_dev, int64_t packed_words, int32_t num_utts, const float* logits,
                          int64_t seq_stride, int64_t frame_stride, int32_t Tpad, int32_t num_classes, int32_t blank, float* grad,
                          int64_t grad_seq_stride, int64_t grad_frame_stride, double* loss, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream_) {
  PK2_REQUIRE(packed && packed_dev && logits && grad && loss && status && workspace, "pk2_ctc_loss_and_grad: null argument");
  PK2_REQUIRE(num_classes >= 2 && blank >= 0 && blank < num_classes, "ctc: blank %d of %d columns", blank, num_classes);
  PK2_REQUIRE(Tpad >= 0 && seq_stride >= 0 && frame_stride >= 0 && grad_seq_stride >= 0 && grad_frame_stride >= 0, "ctc: bad strides");
  size_t ws_words;
  int32_t Tmax, Lmax;
  const int rc = ctc_check(packed, packed_words, num_utts, Tpad, num_classes, blank, &ws_words, &Tmax, &Lmax);
  if (rc != PK2_OK) return rc;
  const size_t need = pk2::align_up(ws_words * 4 + 256, 256);
  PK2_REQUIRE(workspace_bytes >= need, "ctc: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "ctc: the workspace must be 256-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  if (Tmax > 0)
    hipLaunchKernelGGL(ctc_rows, dim3(std::min(256, (Tmax + 3) / 4), num_utts), dim3(256), 0, stream, packed_dev, logits, seq_stride,
                       frame_stride, num_classes, blank, ws);
  hipLaunchKernelGGL(ctc_chains, dim3(2, num_utts), dim3(kThreads), 0, stream, packed_dev, ws, loss, status);
  if (Tpad > 0)
    hipLaunchKernelGGL(ctc_grad, dim3(Tpad, num_utts), dim3(kGradThreads), pk2::align_up(4 * (size_t)(Lmax + 1), 16), stream, packed_dev,
                       logits, seq_stride, frame_stride, num_classes, blank, ws, grad, grad_seq_stride, grad_frame_stride, loss, status);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

}  // extern "C"
