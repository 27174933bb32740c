// The device side that the MBR kernels of lattice_score.hip (one lattice per workgroup, every E-step inside the launch) and
// of lattice_combine.hip (system combination: one E-step per launch and system) share: the launch
// parameters, the view of one (lattice, setting) pair's arrays and workspace, and the E-step itself -- forward, backward
// and statistics passes of DESIGN.md 7.13 on one workgroup of kWsThreads threads.  One source, so one arithmetic: a group of
// one system gives the bits of pk2_wordlat_mbr.  Include after common.h; compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"

namespace pk2 {

constexpr int kWsThreads = 1024;
constexpr int kWsWaves = kWsThreads / 64;
constexpr int kWsPostThreads = 1024;
constexpr int kWsMaxGroups = kWsThreads / 16;   // lane groups of a workgroup at the smallest group width
constexpr double kWsDelta = 1e-5;      // l'(w) = 1 + delta for a word on an arc that the hypothesis does not consume
constexpr double kWsTau = 1e-9;        // tie rule: match, then deletion, then insertion

struct WsParams {
  const int64_t *state_off, *arc_off, *level_off_off, *word_off_off, *post_pre, *mbr_pre, *pe_pre;
  const int32_t *src, *dst, *word, *in_off, *out_off, *out_idx, *level_off, *word_ids, *word_off, *word_arcs;
  const float *graph, *acoustic;
  int32_t first, count, G, with_mbr, kk, bins, decode_mbr, max_iter;
  double* work;
  // best path
  int32_t* bp_words; int32_t bp_stride; int32_t* bp_nwords; double* bp_cost; double* alpha_end; double* post_out;
  int32_t* bp_out; int32_t* post_status;
  // mbr
  int32_t* words; double* conf; int32_t word_stride; int32_t* nwords; double* risk; int32_t* iterations; int32_t* status;
  int32_t* bin_n; int32_t* bin_word; double* bin_post; int32_t bin_stride;
  double set[3 * PK2_WORDLAT_MAX_SETTINGS];
};

struct WsView {
  int S, A, W, depth, cap, P;
  const int32_t *src, *dst, *word, *in_off, *out_off, *out_idx, *level_off, *word_ids, *word_off, *word_arcs;
  const float *graph, *acoustic;
  double *post, *alpha, *v, *Am, *Bm, *Em, *gamma, *part, *topv;
  int32_t *bp, *best, *topw;
  int64_t arc_base, state_base;      // G * (offset of the lattice in the launch's range)
};

// Words (8 bytes) of workspace: per pair [post A | alpha S | v S | bp S, best depth + 2 (int32) | A, B, E S x P | gamma W x P
// | part 64 x P | topv kk x Pe | topw kk x Pe (int32)], Pe = P rounded up to even.
__host__ __device__ inline int64_t ws_post_words(int64_t S, int64_t A, int64_t depth) { return A + 2 * S + (S + depth + 2 + 1) / 2; }
__host__ __device__ inline int64_t ws_mbr_words(int64_t S, int64_t W, int64_t P) { return 3 * S * P + W * P + kWsMaxGroups * P; }

__device__ __forceinline__ WsView ws_view(const WsParams& p, int li, int g) {
  const int l = p.first + li, f = p.first;
  WsView v;
  const int64_t so = p.state_off[l], ao = p.arc_off[l], lo = p.level_off_off[l], wo = p.word_off_off[l];
  v.S = (int)(p.state_off[l + 1] - so);
  v.A = (int)(p.arc_off[l + 1] - ao);
  v.W = (int)(p.word_off_off[l + 1] - wo) - 1;
  v.depth = (int)(p.level_off_off[l + 1] - lo) - 2;
  v.cap = min(PK2_WORDLAT_MAX_POSITIONS, 2 * v.depth + 1);
  v.P = v.cap + 1;
  v.src = p.src + ao; v.dst = p.dst + ao; v.word = p.word + ao; v.graph = p.graph + ao; v.acoustic = p.acoustic + ao;
  v.out_idx = p.out_idx + ao; v.word_arcs = p.word_arcs + ao;
  v.in_off = p.in_off + so + l; v.out_off = p.out_off + so + l;
  v.level_off = p.level_off + lo;
  v.word_off = p.word_off + wo; v.word_ids = p.word_ids + wo - l;
  const int64_t Pe = (v.P + 1) & ~1;
  const int64_t postw = p.post_pre[l + 1] - p.post_pre[l];
  const int64_t mbrw = p.with_mbr ? (p.mbr_pre[l + 1] - p.mbr_pre[l]) + 3 * (int64_t)p.kk * Pe / 2 : 0;
  int64_t before = p.post_pre[l] - p.post_pre[f];
  if (p.with_mbr) before += (p.mbr_pre[l] - p.mbr_pre[f]) + 3 * (int64_t)p.kk * (p.pe_pre[l] - p.pe_pre[f]) / 2;
  double* w = p.work + (int64_t)p.G * before + (int64_t)g * (postw + mbrw);
  v.post = w; v.alpha = v.post + v.A; v.v = v.alpha + v.S;
  v.bp = reinterpret_cast<int32_t*>(v.v + v.S); v.best = v.bp + v.S;
  w += postw;
  v.Am = w; v.Bm = v.Am + (int64_t)v.S * v.P; v.Em = v.Bm + (int64_t)v.S * v.P; v.gamma = v.Em + (int64_t)v.S * v.P;
  v.part = v.gamma + (int64_t)v.W * v.P;
  v.topv = v.part + (int64_t)kWsMaxGroups * v.P; v.topw = reinterpret_cast<int32_t*>(v.topv + (int64_t)p.kk * Pe);
  v.arc_base = (int64_t)p.G * (ao - p.arc_off[f]);
  v.state_base = (int64_t)p.G * (so - p.state_off[f]);
  return v;
}

__device__ __forceinline__ double ws_arc_cost(const WsView& L, int a, double lm, double am, double wip) {
  return lm * (double)L.graph[a] + am * (double)L.acoustic[a] + (L.word[a] != 0 ? wip : 0.0);
}

__device__ __forceinline__ double ws_logadd(double x, double y) {
  const double hi = x >= y ? x : y, lo = x >= y ? y : x;
  return hi + log1p(exp(lo - hi));
}

// ---- MBR ----
struct WsChain { double cmin; int cnt; };   // carried over the chunks of one arc: min over j < 64 c of (t(j) - count(j)); count

// One chunk (q = wd c + sub) of row_a(q) and dec_a(q) of an arc with local word w whose source state has the row Arow, on
// a group of wd = 16, 32 or 64 lanes (sub = lane within the group; the shuffles stay inside the group):
// t = min(a1, a2); the a3 chain row(q-1) + l(0, r_q) is count(q) + min_{j < q} (t(j) - count(j)) with count(q) the number
// of non-zero r_1..r_q, an exact integer.
__device__ __forceinline__ void ws_chunk(const double* Arow, const int32_t* r, int Q, int c, int sub, int wd, int w,
                                         WsChain& ch, double& row, int& dec) {
  const int q = wd * c + sub;
  const bool valid = q <= Q;
  const int rq = (valid && q >= 1) ? r[q] : 0;
  int cnt = rq != 0;
  for (int o = 1; o < wd; o <<= 1) { const int y = __shfl_up(cnt, o, wd); if (sub >= o) cnt += y; }
  cnt += ch.cnt;
  const double lp = w != 0 ? 1.0 + kWsDelta : 0.0;
  const double aq = valid ? Arow[q] : HUGE_VAL, aq1 = (valid && q >= 1) ? Arow[q - 1] : HUGE_VAL;
  const double a2 = aq + lp, a1 = aq1 + (w != rq ? 1.0 : 0.0);
  const double t = fmin(a1, a2);
  double m = t - (double)cnt;
  for (int o = 1; o < wd; o <<= 1) { const double y = __shfl_up(m, o, wd); if (sub >= o) m = fmin(m, y); }
  double ex = __shfl_up(m, 1, wd);
  if (sub == 0) ex = HUGE_VAL;
  ex = fmin(ex, ch.cmin);
  const double a3 = ex + (double)cnt;
  row = fmin(t, a3);
  dec = 0;
  if (valid && q >= 1) dec = (a1 - fmin(a2, a3) <= kWsTau) ? 1 : ((a2 - a3 <= kWsTau) ? 2 : 3);
  ch.cmin = fmin(ch.cmin, __shfl(m, wd - 1, wd));
  ch.cnt = __shfl(cnt, wd - 1, wd);
}

// dec_a and b_a of one arc, chunk by chunk from the top: f(q, valid, dec(q), dec(q+1) or 0 at q >= Q, b(q), b(q+1)).
// b_a(q) = p_a B(n_a, q) + [dec(q+1) = 3] b_a(q+1): a segmented suffix sum over the lanes, the carry from the chunk above.
template <class F>
__device__ __forceinline__ void ws_arc_back(const double* Arow, const double* Bn, const int32_t* r, int Q, int sub, int wd,
                                            int w, double pa, unsigned char* decw, F&& f) {
  const int nc = Q / wd + 1;
  WsChain ch{HUGE_VAL, 0};
  for (int c = 0; c < nc; ++c) {
    double row; int dec;
    ws_chunk(Arow, r, Q, c, sub, wd, w, ch, row, dec);
    decw[wd * c + sub] = (unsigned char)dec;
  }
  double carry_b = 0.0;
  int carry_d = 0;
  for (int c = nc - 1; c >= 0; --c) {
    const int q = wd * c + sub;
    const bool valid = q <= Q;
    const int d = decw[q];
    int dn = __shfl_down(d, 1, wd);
    if (sub == wd - 1) dn = carry_d;
    if (q >= Q) dn = 0;
    double vv = valid ? pa * Bn[q] : 0.0;
    int ff = dn == 3;
    for (int o = 1; o < wd; o <<= 1) {
      const double vo = __shfl_down(vv, o, wd);
      const int fo = __shfl_down(ff, o, wd);
      if (sub + o < wd) { if (ff) vv += vo; ff = ff && fo; }
    }
    if (ff) vv += carry_b;
    double bn = __shfl_down(vv, 1, wd);
    if (sub == wd - 1) bn = carry_b;
    f(q, valid, d, dn, vv, bn);
    carry_b = __shfl(vv, 0, wd);
    carry_d = __shfl(d, 0, wd);
  }
}

__device__ __forceinline__ bool ws_better(double v1, int w1, double v2, int w2) { return v1 > v2 || (v1 == v2 && w1 > w2); }

// One E-step of the workgroup's pair for the hypothesis r (LDS, kWsThreads entries: local word ids at the even positions
// 2 .. Q - 1, 0 elsewhere and behind Q; an id that no arc carries matches nothing and is never used as an index): the rows
// A (risk = A(S - 1, Q)), B, E and gamma(q)[w] for q <= Q in the view's workspace, rows of L.P entries.  decs: kWsWaves *
// kWsThreads bytes of LDS, epart: kWsWaves x 64 doubles of LDS.  Every thread of the workgroup calls it; it ends on a
// barrier, so its results are visible to all of them.
__device__ __forceinline__ void ws_estep(const WsView& L, const int32_t* r, int Q, unsigned char* decs,
                                         double (*epart)[64]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = L.P, S = L.S;
  const int nc = Q / 64 + 1;
  // a hypothesis of Q + 1 <= 16 / 32 positions: groups of 16 / 32 lanes, each on a state (an arc list) of its own
  const int wd = Q + 1 <= 16 ? 16 : (Q + 1 <= 32 ? 32 : 64), sub = tid & (wd - 1), grp = tid / wd, ngrp = kWsThreads / wd;
  const int gnc = Q / wd + 1;
  unsigned char* decw = decs + grp * (kWsThreads / 64) * wd;
  // ---- forward: A(0, q) = number of non-zero r_1..r_q; A(n, .) = sum over the incoming arcs of p_a row_a ----
  for (int64_t i = tid; i < (int64_t)S * P; i += kWsThreads) { L.Bm[i] = 0.0; L.Em[i] = 0.0; }
  if (wave == 0) {
    int carry = 0;
    for (int c = 0; c < nc; ++c) {
      const int q = 64 * c + lane;
      int cnt = (q >= 1 && q <= Q) ? r[q] != 0 : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(cnt, o, 64); if (lane >= o) cnt += y; }
      cnt += carry;
      if (q <= Q) L.Am[q] = (double)cnt;
      carry = __shfl(cnt, 63, 64);
    }
  }
  __syncthreads();
  if (tid == 0) L.Bm[(int64_t)(S - 1) * P + Q] = 1.0;
  // The end state (alone on the last level, an arc from every final state) is summed by all lane groups: group k takes
  // the k-th contiguous slice of its arcs into row k of `part`, thread q adds the rows in group order.
  const int e0 = L.in_off[S - 1], eper = (L.A - e0 + ngrp - 1) / ngrp;
  for (int lev = 1; lev <= L.depth; ++lev) {
    const bool last = lev == L.depth;
    for (int n = L.level_off[lev] + (last ? 0 : grp); n < L.level_off[lev + 1]; n += ngrp) {
      double* An = last ? L.part + (int64_t)grp * P : L.Am + (int64_t)n * P;
      const int a0 = last ? min(L.A, e0 + grp * eper) : L.in_off[n], a1 = last ? min(L.A, a0 + eper) : L.in_off[n + 1];
      for (int a = a0; a < a1; ++a) {
        const double* Arow = L.Am + (int64_t)L.src[a] * P;
        const int w = L.word[a];
        const double pa = L.post[a];
        WsChain ch{HUGE_VAL, 0};
        for (int c = 0; c < gnc; ++c) {
          double row; int dec;
          ws_chunk(Arow, r, Q, c, sub, wd, w, ch, row, dec);
          const int q = wd * c + sub;
          if (q <= Q) An[q] = a == a0 ? pa * row : An[q] + pa * row;
        }
      }
    }
    __syncthreads();
  }
  if (tid <= Q) {
    double acc = L.part[tid];
    for (int k = 1; k < ngrp && e0 + k * eper < L.A; ++k) acc += L.part[(int64_t)k * P + tid];
    L.Am[(int64_t)(S - 1) * P + tid] = acc;
  }
  __syncthreads();
  // ---- backward: B(s, .) and E(s, .) from the outgoing arcs of s, levels descending ----
  for (int lev = L.depth - 1; lev >= 0; --lev) {
    for (int s = L.level_off[lev] + grp; s < L.level_off[lev + 1]; s += ngrp) {
      double* Bs = L.Bm + (int64_t)s * P;
      double* Es = L.Em + (int64_t)s * P;
      const double* Arow = L.Am + (int64_t)s * P;
      for (int k = L.out_off[s]; k < L.out_off[s + 1]; ++k) {
        const int a = L.out_idx[k];
        ws_arc_back(Arow, L.Bm + (int64_t)L.dst[a] * P, r, Q, sub, wd, L.word[a], L.post[a], decw,
                    [&](int q, bool valid, int d, int dn, double b, double bn) {
                      if (!valid) return;
                      double acc = Bs[q];
                      if (q >= 1 && d == 2) acc += b;
                      if (q < Q && dn == 1) acc += bn;
                      if (q == 0) acc += b;
                      Bs[q] = acc;
                      if (q >= 1 && d == 3) Es[q] += b;
                    });
      }
    }
    __syncthreads();
  }
  // ---- statistics: gamma(q)[w], one wave per local word, its arcs in ascending order ----
  // word 0 holds the arcs from the final states: group k takes the k-th slice of its list into row k of `part`
  const int z1 = L.word_off[1], zper = (z1 + ngrp - 1) / ngrp;
  {
    double* Gz = L.part + (int64_t)grp * P;
    for (int c = 0; c < gnc; ++c) { const int q = wd * c + sub; if (q <= Q) Gz[q] = 0.0; }
    for (int k = min(z1, grp * zper); k < min(z1, (grp + 1) * zper); ++k) {
      const int a = L.word_arcs[k];
      ws_arc_back(L.Am + (int64_t)L.src[a] * P, L.Bm + (int64_t)L.dst[a] * P, r, Q, sub, wd, 0, L.post[a], decw,
                  [&](int q, bool valid, int d, int dn, double b, double bn) {
                    if (valid && q >= 1 && d == 1) Gz[q] += b;
                  });
    }
  }
  __syncthreads();
  if (tid <= Q) {
    double acc = 0.0;
    for (int k = 0; k < ngrp; ++k) acc += L.part[(int64_t)k * P + tid];
    L.gamma[tid] = acc;
  }
  for (int w = 1 + grp; w < L.W; w += ngrp) {
    double* Gw = L.gamma + (int64_t)w * P;
    for (int c = 0; c < gnc; ++c) { const int q = wd * c + sub; if (q <= Q) Gw[q] = 0.0; }
    for (int k = L.word_off[w]; k < L.word_off[w + 1]; ++k) {
      const int a = L.word_arcs[k];
      ws_arc_back(L.Am + (int64_t)L.src[a] * P, L.Bm + (int64_t)L.dst[a] * P, r, Q, sub, wd, w, L.post[a], decw,
                  [&](int q, bool valid, int d, int dn, double b, double bn) {
                    if (valid && q >= 1 && d == 1) Gw[q] += b;
                  });
    }
  }
  __syncthreads();
  // word 0: + sum_s E(s, q), + e(q) = sum_{j >= q} B(0, j).  Per chunk: wave k sums its sixteenth of the states in
  // ascending order, the sixteen partial sums are added in wave order.
  for (int c = 0; c < nc; ++c) {
    const int q = 64 * c + lane;
    const bool valid = q <= Q;
    const int per = (S + kWsWaves - 1) / kWsWaves, s0 = wave * per, s1 = min(S, s0 + per);
    double es = 0.0;
    if (valid) for (int s = s0; s < s1; ++s) es += L.Em[(int64_t)s * P + q];
    epart[wave][lane] = es;
    __syncthreads();
    if (wave == 0) {
      es = 0.0;
      for (int k = 0; k < kWsWaves; ++k) es += epart[k][lane];
      double e = valid ? L.Bm[q] : 0.0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const double y = __shfl_down(e, o, 64); if (lane + o < 64) e += y; }
      double tail = 0.0;
      for (int c2 = nc - 1; c2 > c; --c2) {
        const int q2 = 64 * c2 + lane;
        tail += wave_sum_d(q2 <= Q ? L.Bm[q2] : 0.0);
      }
      e += tail;
      if (valid && q >= 1) L.gamma[q] = (L.gamma[q] + es) + e;
    }
    __syncthreads();
  }
}

// The kk highest (posterior, word) of every position 1 .. Q of gamma (W rows of P entries), one wave per position; ties
// go to the larger word id.  topv / topw: Q + 1 rows of kk entries (word -1 where there are fewer than kk words);
// best (LDS): the top word of every position.  The caller's barrier follows.
__device__ __forceinline__ void ws_top_entries(const double* gamma, int W, int P, int Q, int kk, double* topv, int32_t* topw,
                                               int32_t* best) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = 1 + wave; q <= Q; q += kWsWaves) {
    double pv = HUGE_VAL; int pw = W;
    for (int t = 0; t < kk; ++t) {
      double bv = -HUGE_VAL; int bw = -1;
      for (int w = lane; w < W; w += 64) {
        const double x = gamma[(int64_t)w * P + q];
        if (ws_better(pv, pw, x, w) && ws_better(x, w, bv, bw)) { bv = x; bw = w; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64); const int ow = __shfl_xor(bw, o, 64);
        if (ws_better(ov, ow, bv, bw)) { bv = ov; bw = ow; }
      }
      if (lane == 0) { topv[(int64_t)q * kk + t] = bv; topw[(int64_t)q * kk + t] = bw; if (t == 0) best[q] = bw; }
      pv = bv; pw = bw;
      if (bw < 0) { pv = -HUGE_VAL; pw = -1; }
    }
  }
}

struct WordLat;
// ws_post_kernel (lattice_score.hip) for the pairs of lattices first .. first + count - 1 with the workspace layout of a
// best-path-only call (post_pre): post, alpha, v, bp and best of every pair stay in `work`.  Arguments validated by the caller.
int ws_launch_post(const WordLat* h, int first, int count, const double* settings, int G, double* work, hipStream_t stream);
// WsParams of the batch's arrays for a launch over first .. first + count - 1
void ws_fill(const WordLat* h, WsParams& p, int first, int count, const double* settings, int G, bool with_mbr, int bins);
bool ws_settings_ok(const double* s, int G);

}  // namespace pk2
