// Lattice scoring (include/pk2hip.h: pk2_wordlat_*, pk2_edit_distance_batch): arc posteriors and the
// tropical best path of packed word lattices, minimum Bayes risk decoding (Xu, Povey, Mangu, Zhu 2011) with word
// confidences, and Levenshtein distances -- for a grid of (lattice, setting) pairs per launch, setting = (lm, am, wip).
//
//   ws_post_kernel   one workgroup per pair: alpha (log-add), the tropical cost v with back-pointers, level by level with
//                    one thread per state; p_a for every arc; one lane backtraces the best path
//   ws_mbr_kernel    one workgroup of 16 wavefronts per pair, every E-step inside the launch: the lanes sit on the
//                    positions q of the hypothesis in chunks of 64 (groups of 16 or 32 lanes while Q + 1 fits); forward (one wave per state of a level), backward (one
//                    wave per source state), statistics (one wave per word), top entries (one wave per position), update
//   ws_edit_kernel   one wavefront per (hypothesis, reference) pair (lattice_edit.h)
//
// float64 throughout, no floating-point atomics, every sum in a fixed order: the same bits from run to run and in a batch
// as in a single call.  A, B, E (S x P) and gamma (W x P) live in the caller's workspace, P = capacity + 1.
#include <cmath>
#include <vector>

#include "common.h"
#include "lattice_edit.h"
#include "wordlat.h"
#include "wordlat_mbr.h"     // the launch parameters, the view of a pair, the E-step: shared with lattice_combine.hip

#pragma clang fp contract(off)

namespace pk2 {
namespace {

__global__ void __launch_bounds__(kWsPostThreads) ws_post_kernel(WsParams p) {
  const int pair = blockIdx.x, li = pair / p.G, g = pair % p.G, tid = threadIdx.x;
  const WsView L = ws_view(p, li, g);
  const double lm = p.set[3 * g], am = p.set[3 * g + 1], wip = p.set[3 * g + 2];
  if (tid == 0) { L.alpha[0] = 0.0; L.v[0] = 0.0; L.bp[0] = -1; }
  __syncthreads();
  __shared__ double sh_alpha[kWsPostThreads], sh_v[kWsPostThreads];
  __shared__ int32_t sh_arc[kWsPostThreads];
  for (int lev = 1; lev <= L.depth; ++lev) {
    // the end state stands alone on the last level and collects an arc from every final state: thread t takes the t-th
    // contiguous slice of its arcs, thread 0 adds the partial results in slice order
    const bool last = lev == L.depth;
    const int e0 = L.in_off[L.S - 1], per = (L.A - e0 + kWsPostThreads - 1) / kWsPostThreads;
    for (int s = L.level_off[lev] + (last ? 0 : tid); s < L.level_off[lev + 1]; s += kWsPostThreads) {
      double acc = 0.0, vb = HUGE_VAL;
      int barc = -1;
      const int a0 = last ? min(L.A, e0 + tid * per) : L.in_off[s], a1 = last ? min(L.A, a0 + per) : L.in_off[s + 1];
      for (int a = a0; a < a1; ++a) {
        const double cost = ws_arc_cost(L, a, lm, am, wip);
        const int u = L.src[a];
        const double x = L.alpha[u] + (-cost);
        acc = a == a0 ? x : ws_logadd(acc, x);
        const double cand = L.v[u] + cost;
        if (cand < vb || barc < 0) { vb = cand; barc = a; }
      }
      if (!last) { L.alpha[s] = acc; L.v[s] = vb; L.bp[s] = barc; }
      else { sh_alpha[tid] = acc; sh_v[tid] = vb; sh_arc[tid] = barc; }
    }
    __syncthreads();
    if (last && tid == 0) {
      double acc = sh_alpha[0], vb = sh_v[0];
      int barc = sh_arc[0];
      for (int t = 1; t < kWsPostThreads && sh_arc[t] >= 0; ++t) {
        acc = ws_logadd(acc, sh_alpha[t]);
        if (sh_v[t] < vb) { vb = sh_v[t]; barc = sh_arc[t]; }
      }
      L.alpha[L.S - 1] = acc; L.v[L.S - 1] = vb; L.bp[L.S - 1] = barc;
    }
    if (last) __syncthreads();
  }
  for (int a = tid; a < L.A; a += kWsPostThreads) {
    const double cost = ws_arc_cost(L, a, lm, am, wip);
    const double pa = exp(L.alpha[L.src[a]] + (-cost) - L.alpha[L.dst[a]]);
    L.post[a] = pa;
    if (p.post_out) p.post_out[L.arc_base + (int64_t)g * L.A + a] = pa;
  }
  if (p.bp_out) for (int s = tid; s < L.S; s += kWsPostThreads) p.bp_out[L.state_base + (int64_t)g * L.S + s] = L.bp[s];
  if (tid == 0) {
    const double ae = L.alpha[L.S - 1], ve = L.v[L.S - 1];
    const bool ok = isfinite(ae) && isfinite(ve);
    int n = 0;
    if (ok) {
      for (int s = L.S - 1, guard = 0; s > 0 && guard < L.S; ++guard) { const int a = L.bp[s]; n += L.word[a] != 0; s = L.src[a]; }
      int i = n;
      for (int s = L.S - 1, guard = 0; s > 0 && guard < L.S; ++guard) {
        const int a = L.bp[s], w = L.word[a];
        if (w != 0 && i > 0) {
          --i;
          L.best[1 + i] = w;
          if (p.bp_words && i < p.bp_stride) p.bp_words[(int64_t)pair * p.bp_stride + i] = L.word_ids[w];
        }
        s = L.src[a];
      }
    }
    L.best[0] = ok ? n : -1;
    if (p.bp_nwords) p.bp_nwords[pair] = n;
    if (p.bp_cost) p.bp_cost[pair] = ve;
    if (p.alpha_end) p.alpha_end[pair] = ae;
    if (p.post_status) p.post_status[pair] = ok ? 0 : 3;
  }
}

__global__ void __launch_bounds__(kWsThreads) ws_mbr_kernel(WsParams p) {
  __shared__ int32_t r[kWsThreads];
  __shared__ int32_t best[kWsThreads];
  __shared__ unsigned char decs[kWsWaves * kWsThreads];
  __shared__ double epart[kWsWaves][64];
  __shared__ int32_t wave_tot[kWsWaves];
  const int pair = blockIdx.x, li = pair / p.G, g = pair % p.G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WsView L = ws_view(p, li, g);
  const int P = L.P, S = L.S, kk = p.kk;
  const int m0 = L.best[0];
  if (m0 < 0 || 2 * m0 + 1 > L.cap) {       // no path (status 3), or a first hypothesis beyond the row capacity (status 2)
    if (tid == 0) {
      p.nwords[pair] = 0; p.risk[pair] = 0.0; p.iterations[pair] = 0; p.status[pair] = m0 < 0 ? 3 : 2;
      if (p.bin_n) p.bin_n[pair] = 0;
    }
    return;
  }
  r[tid] = 0;
  __syncthreads();
  if (tid < m0) r[2 * (tid + 1)] = L.best[1 + tid];
  int Q = 2 * m0 + 1, iter = 0, status = 0, mnew = 0, idx = 0;
  bool flag = false;
  __syncthreads();
  for (;;) {
    ws_estep(L, r, Q, decs, epart);
    ws_top_entries(L.gamma, L.W, P, Q, kk, L.topv, L.topw, best);
    __syncthreads();
    // ---- decision: thread q looks at position q ----
    ++iter;
    const bool in = tid >= 1 && tid <= Q;
    const int nb = in ? best[tid] : 0;
    flag = in && nb > 0;
    const int changed = __syncthreads_or(in && nb != r[tid]);
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_tot[wave] = __popcll(mask);
    __syncthreads();
    idx = __popcll(mask & ((1ull << lane) - 1ull));
    mnew = 0;
    for (int w2 = 0; w2 < kWsWaves; ++w2) { const int t2 = wave_tot[w2]; if (w2 < wave) idx += t2; mnew += t2; }
    if (!p.decode_mbr || !changed) { status = 0; break; }
    if (iter >= p.max_iter) { status = 1; break; }
    if (2 * mnew + 1 > L.cap) { status = 2; break; }
    __syncthreads();
    r[tid] = 0;
    __syncthreads();
    if (flag) r[2 * (idx + 1)] = nb;
    Q = 2 * mnew + 1;
    __syncthreads();
  }
  // ---- result: the hypothesis of the last E-step with its own statistics ----
  const int m = (Q - 1) / 2;
  if (tid < m && tid < p.word_stride) {
    const int w = r[2 * (tid + 1)];
    p.words[(int64_t)pair * p.word_stride + tid] = L.word_ids[w];
    p.conf[(int64_t)pair * p.word_stride + tid] = L.gamma[(int64_t)w * P + 2 * (tid + 1)];
  }
  if (p.bins > 0 && flag && idx < p.bin_stride) {
    for (int t = 0; t < p.bins; ++t) {
      const int w = L.topw[(int64_t)tid * kk + t];
      const int64_t o = ((int64_t)pair * p.bin_stride + idx) * p.bins + t;
      p.bin_word[o] = w >= 0 ? L.word_ids[w] : -1;
      p.bin_post[o] = w >= 0 ? L.topv[(int64_t)tid * kk + t] : 0.0;
    }
  }
  if (tid == 0) {
    p.nwords[pair] = m; p.risk[pair] = L.Am[(int64_t)(S - 1) * P + Q]; p.iterations[pair] = iter; p.status[pair] = status;
    if (p.bin_n) p.bin_n[pair] = mnew;
  }
}

// ---- word times ----
struct WsTimes {
  const int32_t* state_time;   // frame of every state, laid out like state_off
  int64_t base;                // words of `work` in front of the times area: the MBR workspace of the launch
  double* times; double* bin_times; int32_t* path_times; int32_t path_stride;
};

// Words of the times area per pair: [TB 64 x Pe | TE 64 x Pe | wanted W + 1 (int32, one word each for a simple prefix)]
__host__ __device__ inline int64_t ws_times_words(int64_t W, int64_t Pe) { return 2 * kWsMaxGroups * Pe + (W + 1); }

// After ws_mbr_kernel, on the workspace it leaves behind (A, B, gamma, topw of the last E-step; bp and best of
// ws_post_kernel): TB(q)[w] = sum over the arcs of w of [dec_a(q) = 1] t(s_a) b_a(q), TE with t(n_a), for the words the
// record reports; begin = TB / gamma, end = TE / gamma.  One lane group per wanted word, the arcs of the word in the order
// and with the group widths of the statistics pass; the lane that owns q keeps TB(q), TE(q) in its group's row and
// divides.  Thread 0 walks the back-pointers for the best path's own arc times.
__global__ void __launch_bounds__(kWsThreads) ws_times_kernel(WsParams p, WsTimes x) {
  __shared__ int32_t r[kWsThreads];
  __shared__ int32_t bidx[kWsThreads];
  __shared__ unsigned char decs[kWsWaves * kWsThreads];
  __shared__ int32_t wave_tot[kWsWaves];
  const int pair = blockIdx.x, li = pair / p.G, g = pair % p.G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WsView L = ws_view(p, li, g);
  const int l = p.first + li, P = L.P, kk = p.kk;
  const int32_t* T = x.state_time + p.state_off[l];
  const int m0 = L.best[0];
  // ---- the best path's word arcs; the rows behind them are (-1, -1) ----
  int32_t* pt = x.path_times + 2 * (int64_t)pair * x.path_stride;
  for (int k = max(m0, 0) + tid; k < x.path_stride; k += kWsThreads) { pt[2 * k] = -1; pt[2 * k + 1] = -1; }
  if (tid == 0 && m0 > 0) {
    int i = m0;
    for (int s = L.S - 1, guard = 0; s > 0 && guard < L.S; ++guard) {
      const int a = L.bp[s];
      if (L.word[a] != 0 && i > 0) {
        --i;
        if (i < x.path_stride) { pt[2 * i] = T[L.src[a]]; pt[2 * i + 1] = T[L.dst[a]]; }
      }
      s = L.src[a];
    }
  }
  if (m0 < 0 || 2 * m0 + 1 > L.cap) return;      // ws_mbr_kernel ran no E-step
  // ---- the hypothesis of the last E-step, from the words it reported ----
  const int m = max(0, min(p.nwords[pair], (L.cap - 1) / 2)), Q = 2 * m + 1;
  const int64_t Pe = (P + 1) & ~1;
  double* tw = p.work + x.base + (int64_t)p.G * (2 * kWsMaxGroups * (p.pe_pre[l] - p.pe_pre[p.first]) +
                                                 (p.word_off_off[l] - p.word_off_off[p.first])) +
               (int64_t)g * ws_times_words(L.W, Pe);
  int32_t* want = reinterpret_cast<int32_t*>(tw + 2 * kWsMaxGroups * Pe);
  r[tid] = 0;
  bidx[tid] = -1;
  for (int w = tid; w < L.W; w += kWsThreads) want[w] = 0;
  __syncthreads();
  if (tid < m) {
    const int gid = p.words[(int64_t)pair * p.word_stride + tid];
    int lo = 0, hi = L.W - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (L.word_ids[mid] < gid) lo = mid + 1; else hi = mid; }
    r[2 * (tid + 1)] = lo;
    want[lo] = 1;
    x.times[2 * ((int64_t)pair * p.word_stride + tid)] = -1.0;
    x.times[2 * ((int64_t)pair * p.word_stride + tid) + 1] = -1.0;
  }
  // ---- the bins: position q is reported when its best word is not epsilon, at the rank ws_mbr_kernel gave it ----
  if (p.bins > 0) {
    const bool flag = tid >= 1 && tid <= Q && L.topw[(int64_t)tid * kk] > 0;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_tot[wave] = __popcll(mask);
    __syncthreads();
    int idx = __popcll(mask & ((1ull << lane) - 1ull));
    for (int w2 = 0; w2 < wave; ++w2) idx += wave_tot[w2];
    if (flag && idx < p.bin_stride) {
      bidx[tid] = idx;
      for (int t = 0; t < p.bins; ++t) {
        const int w = L.topw[(int64_t)tid * kk + t];
        if (w > 0) want[w] = 1;
        const int64_t o = 2 * (((int64_t)pair * p.bin_stride + idx) * p.bins + t);
        x.bin_times[o] = -1.0; x.bin_times[o + 1] = -1.0;
      }
    }
  }
  __syncthreads();
  // ---- the wanted words ----
  const int wd = Q + 1 <= 16 ? 16 : (Q + 1 <= 32 ? 32 : 64), sub = tid & (wd - 1), grp = tid / wd, ngrp = kWsThreads / wd;
  const int gnc = Q / wd + 1;
  unsigned char* decw = decs + grp * (kWsThreads / 64) * wd;
  double* TBg = tw + (int64_t)grp * P;
  double* TEg = tw + (int64_t)(kWsMaxGroups + grp) * P;
  for (int w = 1 + grp; w < L.W; w += ngrp) {
    if (!want[w]) continue;
    for (int c = 0; c < gnc; ++c) { const int q = wd * c + sub; if (q <= Q) { TBg[q] = 0.0; TEg[q] = 0.0; } }
    for (int k = L.word_off[w]; k < L.word_off[w + 1]; ++k) {
      const int a = L.word_arcs[k];
      const double ts = (double)T[L.src[a]], tn = (double)T[L.dst[a]];
      ws_arc_back(L.Am + (int64_t)L.src[a] * P, L.Bm + (int64_t)L.dst[a] * P, r, Q, sub, wd, w, L.post[a], decw,
                  [&](int q, bool valid, int d, int dn, double b, double bn) {
                    if (valid && q >= 1 && d == 1) { TBg[q] += ts * b; TEg[q] += tn * b; }
                  });
    }
    for (int c = 0; c < gnc; ++c) {
      const int q = wd * c + sub;
      if (q < 1 || q > Q) continue;
      const double gm = L.gamma[(int64_t)w * P + q];
      const double tb = gm > 0.0 ? TBg[q] / gm : -1.0, te = gm > 0.0 ? TEg[q] / gm : -1.0;
      if (r[q] == w) {
        const int64_t o = 2 * ((int64_t)pair * p.word_stride + (q / 2 - 1));
        x.times[o] = tb; x.times[o + 1] = te;
      }
      const int idx = bidx[q];
      if (idx >= 0) {
        for (int t = 0; t < p.bins; ++t) {
          if (L.topw[(int64_t)q * kk + t] != w) continue;
          const int64_t o = 2 * (((int64_t)pair * p.bin_stride + idx) * p.bins + t);
          x.bin_times[o] = tb; x.bin_times[o + 1] = te;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(64) ws_edit_kernel(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref,
                                                     const int64_t* ref_off, int32_t* out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int a = (int)(hyp_off[n + 1] - hyp_off[n]), b = (int)(ref_off[n + 1] - ref_off[n]);
  if (b > 64 * kEdChunks - 1 || a < 0 || b < 0) { if (lane == 0) out[n] = -1; return; }
  const int e = edit_wave(hyp + hyp_off[n], a, ref + ref_off[n], b, lane);
  if (lane == 0) out[n] = e;
}

}  // namespace

// ---- host ----
void ws_fill(const WordLat* h, WsParams& p, int first, int count, const double* settings, int G, bool with_mbr, int bins) {
  memset(&p, 0, sizeof(p));
  p.state_off = h->d_state_off; p.arc_off = h->d_arc_off; p.level_off_off = h->d_level_off_off;
  p.word_off_off = h->d_word_off_off; p.post_pre = h->d_post_pre; p.mbr_pre = h->d_mbr_pre; p.pe_pre = h->d_pe_pre;
  p.src = h->d_src; p.dst = h->d_dst; p.word = h->d_word; p.in_off = h->d_in_off; p.out_off = h->d_out_off;
  p.out_idx = h->d_out_idx; p.level_off = h->d_level_off; p.word_ids = h->d_word_ids; p.word_off = h->d_word_off;
  p.word_arcs = h->d_word_arcs; p.graph = h->d_graph; p.acoustic = h->d_acoustic;
  p.first = first; p.count = count; p.G = G; p.with_mbr = with_mbr; p.kk = bins > 1 ? bins : 1; p.bins = bins;
  for (int i = 0; i < 3 * G; ++i) p.set[i] = settings[i];
}

bool ws_settings_ok(const double* s, int G) {
  for (int i = 0; i < 3 * G; ++i) if (!std::isfinite(s[i])) return false;
  return true;
}

int ws_launch_post(const WordLat* h, int first, int count, const double* settings, int G, double* work, hipStream_t stream) {
  WsParams p;
  ws_fill(h, p, first, count, settings, G, false, 0);
  p.work = work;
  hipLaunchKernelGGL(ws_post_kernel, dim3(count * G), dim3(kWsPostThreads), 0, stream, p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

namespace {

size_t ws_bytes(const WordLat* h, int first, int count, int G, int bins) {
  int64_t w = h->post_pre[first + count] - h->post_pre[first];
  if (bins >= 0) {
    const int64_t kk = bins > 1 ? bins : 1;
    w += (h->mbr_pre[first + count] - h->mbr_pre[first]) + 3 * kk * (h->pe_pre[first + count] - h->pe_pre[first]) / 2;
  }
  return (size_t)(w * G) * 8;
}

size_t ws_times_bytes(const WordLat* h, int first, int count, int G, int bins) {
  const int64_t w = 2 * kWsMaxGroups * (h->pe_pre[first + count] - h->pe_pre[first]) +
                    (h->word_off_off[first + count] - h->word_off_off[first]);
  return ws_bytes(h, first, count, G, bins) + (size_t)(w * G) * 8;
}

bool ws_range_ok(const WordLat* h, int first, int count) {
  return h && first >= 0 && count >= 1 && (int64_t)first + count <= h->N;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" int pk2_wordlat_create(int32_t N, const int64_t* state_off, const int64_t* arc_off, const int64_t* level_off_off,
                                  const int64_t* word_off_off, const int32_t* src, const int32_t* dst, const int32_t* word,
                                  const float* graph, const float* acoustic, const int32_t* in_off, const int32_t* out_off,
                                  const int32_t* out_idx, const int32_t* level_off, const int32_t* word_ids,
                                  const int32_t* word_off, const int32_t* word_arcs, void* stream, void** out) {
  PK2_REQUIRE(out, "wordlat_create: null output");
  *out = nullptr;
  PK2_REQUIRE(N >= 1 && state_off && arc_off && level_off_off && word_off_off && src && dst && word && graph && acoustic && in_off &&
              out_off && out_idx && level_off && word_ids && word_off && word_arcs, "wordlat_create: null pointer or no lattice");
  PK2_REQUIRE(state_off[0] == 0 && arc_off[0] == 0 && level_off_off[0] == 0 && word_off_off[0] == 0,
              "wordlat_create: offsets must start at 0");
  WordLat* h = new WordLat;
  h->N = N;
  h->state_off.assign(state_off, state_off + N + 1); h->arc_off.assign(arc_off, arc_off + N + 1);
  h->level_off_off.assign(level_off_off, level_off_off + N + 1); h->word_off_off.assign(word_off_off, word_off_off + N + 1);
  h->post_pre.assign(N + 1, 0); h->mbr_pre.assign(N + 1, 0); h->pe_pre.assign(N + 1, 0);
  h->depth.resize(N); h->cap.resize(N);
  // every index the kernels follow is checked here, once
  const char* bad = nullptr;
  for (int l = 0; l < N && !bad; ++l) {
    const int64_t S = state_off[l + 1] - state_off[l], A = arc_off[l + 1] - arc_off[l];
    const int64_t D = level_off_off[l + 1] - level_off_off[l] - 2, W = word_off_off[l + 1] - word_off_off[l] - 1;
    if (S < 2 || A < 1 || D < 1 || W < 1 || S > (1 << 30) || A > (1 << 30)) { bad = "sizes"; break; }
    const int32_t *s_ = src + arc_off[l], *d_ = dst + arc_off[l], *w_ = word + arc_off[l], *oi = out_idx + arc_off[l];
    const int32_t *wa = word_arcs + arc_off[l];
    const int32_t *io = in_off + state_off[l] + l, *oo = out_off + state_off[l] + l, *lo = level_off + level_off_off[l];
    const int32_t *wo = word_off + word_off_off[l], *wi = word_ids + word_off_off[l] - l;
    if (lo[0] != 0 || lo[1] != 1 || lo[D + 1] != S || lo[D] != S - 1) { bad = "level ranges"; break; }
    std::vector<int32_t> lev(S);
    for (int64_t v = 0; v <= D && !bad; ++v) {
      if (lo[v + 1] <= lo[v]) { bad = "level ranges"; break; }
      for (int32_t s = lo[v]; s < lo[v + 1]; ++s) lev[s] = (int32_t)v;
    }
    if (bad) break;
    if (io[0] != 0 || io[S] != A || oo[0] != 0 || oo[S] != A || wo[0] != 0 || wo[W] != A || wi[0] != 0) { bad = "offsets"; break; }
    for (int64_t s = 0; s < S; ++s) if (io[s + 1] < io[s] || oo[s + 1] < oo[s]) bad = "offsets";
    for (int64_t w = 0; w < W; ++w) if (wo[w + 1] < wo[w] || (w > 0 && wi[w] <= wi[w - 1])) bad = "word map";
    if (bad) break;
    if (io[1] != 0) { bad = "start state has incoming arcs"; break; }
    for (int64_t s = 1; s < S; ++s) if (io[s + 1] == io[s]) bad = "state without incoming arc";
    for (int64_t s = 0; s + 1 < S; ++s) if (oo[s + 1] == oo[s]) bad = "state without outgoing arc";
    if (bad) break;
    for (int64_t s = 0; s < S && !bad; ++s) {
      for (int32_t a = io[s]; a < io[s + 1]; ++a) if (d_[a] != s) bad = "arcs not sorted by destination";
      for (int32_t k = oo[s]; k < oo[s + 1]; ++k) {
        if (oi[k] < 0 || oi[k] >= A || s_[oi[k]] != s || (k > oo[s] && oi[k] <= oi[k - 1])) { bad = "source index"; break; }
      }
    }
    for (int64_t a = 0; a < A && !bad; ++a) {
      if (s_[a] < 0 || s_[a] >= S || d_[a] < 0 || d_[a] >= S || lev[s_[a]] >= lev[d_[a]]) bad = "arc does not go up a level";
      else if (w_[a] < 0 || w_[a] >= W) bad = "word id";
      else if (!std::isfinite(graph[arc_off[l] + a]) || !std::isfinite(acoustic[arc_off[l] + a])) bad = "non-finite cost";
    }
    for (int64_t w = 0; w < W && !bad; ++w)
      for (int32_t k = wo[w]; k < wo[w + 1]; ++k)
        if (wa[k] < 0 || wa[k] >= A || w_[wa[k]] != w || (k > wo[w] && wa[k] <= wa[k - 1])) { bad = "word arc list"; break; }
    const int64_t cap = std::min<int64_t>(PK2_WORDLAT_MAX_POSITIONS, 2 * D + 1), P = cap + 1;
    h->depth[l] = (int32_t)D; h->cap[l] = (int32_t)cap;
    h->h_src.insert(h->h_src.end(), s_, s_ + A); h->h_dst.insert(h->h_dst.end(), d_, d_ + A);
    h->h_word_ids.insert(h->h_word_ids.end(), wi, wi + W);
    h->post_pre[l + 1] = h->post_pre[l] + ws_post_words(S, A, D);
    h->mbr_pre[l + 1] = h->mbr_pre[l] + ws_mbr_words(S, W, P);
    h->pe_pre[l + 1] = h->pe_pre[l] + ((P + 1) & ~(int64_t)1);
  }
  if (bad) {
    delete h;
    set_error("wordlat_create: malformed packed lattice (%s)", bad);
    return PK2_ERR_INVALID;
  }
  const size_t TA = (size_t)arc_off[N], TS = (size_t)state_off[N] + N, TL = (size_t)level_off_off[N], TW = (size_t)word_off_off[N];
  Carver sz(nullptr);
  auto carve = [&](Carver& c, WordLat* o) {
    o->d_state_off = c.take<int64_t>(N + 1); o->d_arc_off = c.take<int64_t>(N + 1); o->d_level_off_off = c.take<int64_t>(N + 1);
    o->d_word_off_off = c.take<int64_t>(N + 1); o->d_post_pre = c.take<int64_t>(N + 1); o->d_mbr_pre = c.take<int64_t>(N + 1);
    o->d_pe_pre = c.take<int64_t>(N + 1);
    o->d_src = c.take<int32_t>(TA); o->d_dst = c.take<int32_t>(TA); o->d_word = c.take<int32_t>(TA);
    o->d_out_idx = c.take<int32_t>(TA); o->d_word_arcs = c.take<int32_t>(TA);
    o->d_graph = c.take<float>(TA); o->d_acoustic = c.take<float>(TA);
    o->d_in_off = c.take<int32_t>(TS); o->d_out_off = c.take<int32_t>(TS); o->d_level_off = c.take<int32_t>(TL);
    o->d_word_off = c.take<int32_t>(TW); o->d_word_ids = c.take<int32_t>(TW - N);
  };
  WordLat dummy;
  carve(sz, &dummy);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMalloc(&h->blob, sz.bytes());
  if (e != hipSuccess) { delete h; set_error("wordlat_create: hipMalloc(%zu) -> %s", sz.bytes(), hipGetErrorString(e)); return PK2_ERR_HIP; }
  Carver cv(h->blob);
  carve(cv, h);
  auto up = [&](const void* d, const void* s, size_t n) { if (e == hipSuccess && n) e = hipMemcpyAsync(const_cast<void*>(d), s, n, hipMemcpyHostToDevice, st); };
  up(h->d_state_off, state_off, 8 * (N + 1)); up(h->d_arc_off, arc_off, 8 * (N + 1)); up(h->d_level_off_off, level_off_off, 8 * (N + 1));
  up(h->d_word_off_off, word_off_off, 8 * (N + 1)); up(h->d_post_pre, h->post_pre.data(), 8 * (N + 1));
  up(h->d_mbr_pre, h->mbr_pre.data(), 8 * (N + 1)); up(h->d_pe_pre, h->pe_pre.data(), 8 * (N + 1));
  up(h->d_src, src, 4 * TA); up(h->d_dst, dst, 4 * TA); up(h->d_word, word, 4 * TA); up(h->d_out_idx, out_idx, 4 * TA);
  up(h->d_word_arcs, word_arcs, 4 * TA); up(h->d_graph, graph, 4 * TA); up(h->d_acoustic, acoustic, 4 * TA);
  up(h->d_in_off, in_off, 4 * TS); up(h->d_out_off, out_off, 4 * TS); up(h->d_level_off, level_off, 4 * TL);
  up(h->d_word_off, word_off, 4 * TW); up(h->d_word_ids, word_ids, 4 * (TW - N));
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(h->blob);
    delete h;
    set_error("wordlat_create: upload -> %s", hipGetErrorString(e));
    return PK2_ERR_HIP;
  }
  *out = h;
  return PK2_OK;
}

extern "C" int pk2_wordlat_destroy(void* handle) {
  WordLat* h = static_cast<WordLat*>(handle);
  if (!h) return PK2_OK;
  if (h->d_state_time) (void)hipFree(h->d_state_time);
  if (h->gblob) (void)hipFree(h->gblob);
  if (h->sblob) (void)hipFree(h->sblob);
  if (h->blob) PK2_HIP(hipFree(h->blob));
  delete h;
  return PK2_OK;
}

extern "C" size_t pk2_wordlat_workspace_bytes(const void* handle, int32_t first, int32_t count, int32_t G, int32_t bins) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  if (!ws_range_ok(h, first, count) || G < 1 || G > PK2_WORDLAT_MAX_SETTINGS || bins < -1 || bins > PK2_WORDLAT_MAX_BINS) return 0;
  return ws_bytes(h, first, count, G, bins);
}

extern "C" int pk2_wordlat_best_path(const void* handle, int32_t first, int32_t count, const double* settings, int32_t G,
                                     void* work, size_t work_bytes, int32_t* words, int32_t word_stride, int32_t* nwords,
                                     double* cost, double* alpha_end, double* post, int32_t* backpointer, int32_t* status,
                                     void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && settings && work && words && nwords && cost && alpha_end && status, "wordlat_best_path: null pointer");
  PK2_REQUIRE(G >= 1 && G <= PK2_WORDLAT_MAX_SETTINGS, "wordlat_best_path: %d settings (1..%d)", G, PK2_WORDLAT_MAX_SETTINGS);
  PK2_REQUIRE(ws_settings_ok(settings, G), "wordlat_best_path: non-finite scale");
  PK2_REQUIRE(ws_range_ok(h, first, count), "wordlat_best_path: lattices %d..%d of %d", first, first + count, h->N);
  for (int l = first; l < first + count; ++l)
    PK2_REQUIRE(word_stride >= h->depth[l], "wordlat_best_path: word_stride %d below the depth %d of lattice %d", word_stride, h->depth[l], l);
  PK2_REQUIRE(work_bytes >= ws_bytes(h, first, count, G, -1) && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_best_path: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, ws_bytes(h, first, count, G, -1));
  WsParams p;
  ws_fill(h, p, first, count, settings, G, false, 0);
  p.work = static_cast<double*>(work);
  p.bp_words = words; p.bp_stride = word_stride; p.bp_nwords = nwords; p.bp_cost = cost; p.alpha_end = alpha_end;
  p.post_out = post; p.bp_out = backpointer; p.post_status = status;
  hipLaunchKernelGGL(ws_post_kernel, dim3(count * G), dim3(kWsPostThreads), 0, static_cast<hipStream_t>(stream), p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_wordlat_mbr(const void* handle, int32_t first, int32_t count, const double* settings, int32_t G,
                               int32_t decode_mbr, int32_t max_iter, int32_t bins, void* work, size_t work_bytes, int32_t* words,
                               double* conf, int32_t word_stride, int32_t* nwords, double* risk, int32_t* iterations,
                               int32_t* status, int32_t* bin_n, int32_t* bin_word, double* bin_post, int32_t bin_stride,
                               void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && settings && work && words && conf && nwords && risk && iterations && status, "wordlat_mbr: null pointer");
  PK2_REQUIRE(G >= 1 && G <= PK2_WORDLAT_MAX_SETTINGS, "wordlat_mbr: %d settings (1..%d)", G, PK2_WORDLAT_MAX_SETTINGS);
  PK2_REQUIRE(bins >= 0 && bins <= PK2_WORDLAT_MAX_BINS, "wordlat_mbr: bins %d (0..%d)", bins, PK2_WORDLAT_MAX_BINS);
  PK2_REQUIRE(bins == 0 || (bin_n && bin_word && bin_post), "wordlat_mbr: null pointer for the bins");
  PK2_REQUIRE(max_iter >= 1, "wordlat_mbr: max_iter %d", max_iter);
  PK2_REQUIRE(ws_settings_ok(settings, G), "wordlat_mbr: non-finite scale");
  PK2_REQUIRE(ws_range_ok(h, first, count), "wordlat_mbr: lattices %d..%d of %d", first, first + count, h->N);
  for (int l = first; l < first + count; ++l) {
    PK2_REQUIRE(word_stride >= (h->cap[l] - 1) / 2, "wordlat_mbr: word_stride %d, lattice %d can hold %d words", word_stride, l,
                (h->cap[l] - 1) / 2);
    PK2_REQUIRE(bins == 0 || bin_stride >= h->cap[l], "wordlat_mbr: bin_stride %d below the capacity %d of lattice %d", bin_stride,
                h->cap[l], l);
  }
  PK2_REQUIRE(work_bytes >= ws_bytes(h, first, count, G, bins) && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_mbr: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, ws_bytes(h, first, count, G, bins));
  WsParams p;
  ws_fill(h, p, first, count, settings, G, true, bins);
  p.work = static_cast<double*>(work);
  p.decode_mbr = decode_mbr != 0; p.max_iter = max_iter;
  p.words = words; p.conf = conf; p.word_stride = word_stride; p.nwords = nwords; p.risk = risk; p.iterations = iterations;
  p.status = status; p.bin_n = bins ? bin_n : nullptr; p.bin_word = bin_word; p.bin_post = bin_post; p.bin_stride = bin_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ws_post_kernel, dim3(count * G), dim3(kWsPostThreads), 0, st, p);
  PK2_LAUNCH_CHECK();
  hipLaunchKernelGGL(ws_mbr_kernel, dim3(count * G), dim3(kWsThreads), 0, st, p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_wordlat_set_times(void* handle, const int32_t* state_time) {
  WordLat* h = static_cast<WordLat*>(handle);
  PK2_REQUIRE(h && state_time, "wordlat_set_times: null pointer");
  PK2_REQUIRE(h->N >= 1, "wordlat_set_times: not a batch of pk2_wordlat_create");
  for (int l = 0; l < h->N; ++l) {
    const int32_t* t = state_time + h->state_off[l];
    PK2_REQUIRE(t[0] == 0, "wordlat_set_times: lattice %d starts at frame %d, not 0", l, t[0]);
    for (int64_t a = h->arc_off[l]; a < h->arc_off[l + 1]; ++a)
      PK2_REQUIRE(t[h->h_dst[a]] >= t[h->h_src[a]], "wordlat_set_times: lattice %d, arc %lld has the negative length %d", l,
                  (long long)(a - h->arc_off[l]), t[h->h_dst[a]] - t[h->h_src[a]]);
  }
  const size_t bytes = 4 * (size_t)h->state_off[h->N];
  if (!h->d_state_time) PK2_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_state_time), bytes));
  PK2_HIP(hipMemcpy(h->d_state_time, state_time, bytes, hipMemcpyHostToDevice));
  return PK2_OK;
}

extern "C" size_t pk2_wordlat_times_workspace_bytes(const void* handle, int32_t first, int32_t count, int32_t G, int32_t bins) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  if (!ws_range_ok(h, first, count) || G < 1 || G > PK2_WORDLAT_MAX_SETTINGS || bins < 0 || bins > PK2_WORDLAT_MAX_BINS) return 0;
  return ws_times_bytes(h, first, count, G, bins);
}

extern "C" int pk2_wordlat_mbr_times(const void* handle, int32_t first, int32_t count, const double* settings, int32_t G,
                                     int32_t decode_mbr, int32_t max_iter, int32_t bins, void* work, size_t work_bytes,
                                     int32_t* words, double* conf, int32_t word_stride, int32_t* nwords, double* risk,
                                     int32_t* iterations, int32_t* status, int32_t* bin_n, int32_t* bin_word, double* bin_post,
                                     int32_t bin_stride, double* times, double* bin_times, int32_t* path_times,
                                     int32_t path_stride, void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && times && path_times, "wordlat_mbr_times: null pointer");
  PK2_REQUIRE(h->d_state_time, "wordlat_mbr_times: no state times (pk2_wordlat_set_times comes first)");
  PK2_REQUIRE(bins >= 0 && bins <= PK2_WORDLAT_MAX_BINS, "wordlat_mbr_times: bins %d (0..%d)", bins, PK2_WORDLAT_MAX_BINS);
  PK2_REQUIRE(bins == 0 || bin_times, "wordlat_mbr_times: null pointer for the bin times");
  PK2_REQUIRE(G >= 1 && G <= PK2_WORDLAT_MAX_SETTINGS, "wordlat_mbr_times: %d settings (1..%d)", G, PK2_WORDLAT_MAX_SETTINGS);
  PK2_REQUIRE(ws_range_ok(h, first, count), "wordlat_mbr_times: lattices %d..%d of %d", first, first + count, h->N);
  for (int l = first; l < first + count; ++l)
    PK2_REQUIRE(path_stride >= h->depth[l], "wordlat_mbr_times: path_stride %d below the depth %d of lattice %d", path_stride,
                h->depth[l], l);
  PK2_REQUIRE(work_bytes >= ws_times_bytes(h, first, count, G, bins), "wordlat_mbr_times: workspace of %zu bytes, need %zu",
              work_bytes, ws_times_bytes(h, first, count, G, bins));
  // the remaining arguments are pk2_wordlat_mbr's and are checked there, before its first launch
  const int rc = pk2_wordlat_mbr(handle, first, count, settings, G, decode_mbr, max_iter, bins, work, work_bytes, words, conf,
                                 word_stride, nwords, risk, iterations, status, bin_n, bin_word, bin_post, bin_stride, stream);
  if (rc != PK2_OK) return rc;
  WsParams p;
  ws_fill(h, p, first, count, settings, G, true, bins);
  p.work = static_cast<double*>(work);
  p.words = words; p.word_stride = word_stride; p.nwords = nwords; p.bin_stride = bin_stride;
  WsTimes x;
  x.state_time = h->d_state_time; x.base = (int64_t)(ws_bytes(h, first, count, G, bins) / 8);
  x.times = times; x.bin_times = bin_times; x.path_times = path_times; x.path_stride = path_stride;
  hipLaunchKernelGGL(ws_times_kernel, dim3(count * G), dim3(kWsThreads), 0, static_cast<hipStream_t>(stream), p, x);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_edit_distance_batch(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off,
                                       int32_t n, int32_t* out, void* stream) {
  PK2_REQUIRE(hyp && hyp_off && ref && ref_off && out, "edit_distance_batch: null pointer");
  PK2_REQUIRE(n >= 0, "edit_distance_batch: n = %d", n);
  if (n == 0) return PK2_OK;
  hipLaunchKernelGGL(ws_edit_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), hyp, hyp_off, ref, ref_off, out);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
