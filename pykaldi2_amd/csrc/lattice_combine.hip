// MBR system combination of word lattices (include/pk2hip.h: pk2_wordlat_set_groups, pk2_wordlat_combine):
// what the reference's score_combine.sh hands to Kaldi's lattice-combine | lattice-mbr-decode.  A group holds the K <= 8
// lattices that K systems made of one utterance; the union's path distribution is sum_k wn_k P_k and the MBR statistics are
// linear in it, so no union lattice is built: every system runs the E-step of lattice_score.hip (wordlat_mbr.h: one source,
// one arithmetic) on its own lattice, and a small kernel per (group, setting) adds the statistics and decides.
//
//   ws_post_kernel     (lattice_score.hip) once per (lattice, setting): p_a, alpha, v, the best path
//   wc_init_kernel     one workgroup per (group, setting): the system whose best path has the highest normalised weight
//                      wn_k exp(-v_k) / exp(Z_k) starts; its words go to R in the group's union vocabulary
//   wc_estep_kernel    one workgroup of 16 wavefronts per (lattice, setting): R through the system's map into LDS, then
//                      ws_estep; risk_k = A_k(end, Q) and gamma_k stay in its workspace
//   wc_update_kernel   one workgroup per (group, setting): Gamma = sum_k wn_k gamma_k in ascending k, the top entries, the
//                      decision, the new R; a pair that stops writes its outputs and sets its `done` flag
//
// max_iter rounds of (wc_estep_kernel, wc_update_kernel) are enqueued without a read-back; the workgroups of a pair that is
// done return at once.  float64, no floating-point atomics, fixed summation orders, no workgroup waits for another.
#include <cmath>
#include <vector>

#include "common.h"
#include "wordlat.h"
#include "wordlat_mbr.h"

#pragma clang fp contract(off)

namespace pk2 {
namespace {

constexpr int kWcMaxSystems = PK2_WORDLAT_MAX_SYSTEMS;
constexpr int kWcStateWords = 8 + kWsThreads / 2;   // words of a pair's state: header (int32 Q, iterations, done, system), R

struct WcParams {
  const int32_t *group_off, *lat_group, *gcap, *uvoc, *map;
  const double *wn, *logwn;
  const int64_t *uvoc_off, *map_off, *est_pre, *grp_pre, *gpe_pre;
  int32_t g0, gcount;
  int64_t est_base, grp_base;       // words of `work` in front of the E-step area and of the groups' area
  int32_t* system;
};

// The (group, setting) pair's own area: [Gamma WU x P | header, R | topv kk x Pe | topw kk x Pe (int32)]
struct WcGroup {
  int WU, cap, P, l0, K;
  double *Gamma, *topv;
  int32_t *hd, *R, *topw;
  const int32_t* uvoc;
};

__device__ __forceinline__ WcGroup wc_group(const WsParams& p, const WcParams& x, int gi, int g) {
  WcGroup o;
  o.l0 = x.group_off[gi]; o.K = x.group_off[gi + 1] - o.l0;
  o.WU = (int)(x.uvoc_off[gi + 1] - x.uvoc_off[gi]);
  o.uvoc = x.uvoc + x.uvoc_off[gi];
  o.cap = x.gcap[gi]; o.P = o.cap + 1;
  const int64_t Pe = (o.P + 1) & ~1;
  const int64_t words = (x.grp_pre[gi + 1] - x.grp_pre[gi]) + 3 * (int64_t)p.kk * Pe / 2;
  const int64_t before = (x.grp_pre[gi] - x.grp_pre[x.g0]) + 3 * (int64_t)p.kk * (x.gpe_pre[gi] - x.gpe_pre[x.g0]) / 2;
  double* w = p.work + x.grp_base + (int64_t)p.G * before + (int64_t)g * words;
  o.Gamma = w;
  o.hd = reinterpret_cast<int32_t*>(w + (int64_t)o.WU * o.P); o.R = o.hd + 16;
  o.topv = w + (int64_t)o.WU * o.P + kWcStateWords;
  o.topw = reinterpret_cast<int32_t*>(o.topv + (int64_t)p.kk * Pe);
  return o;
}

// The view of lattice l = p.first + li at setting g with the rows of its group: post, alpha, v, bp, best where
// ws_post_kernel left them, A, B, E, gamma, part in the E-step area.
__device__ __forceinline__ WsView wc_view(const WsParams& p, const WcParams& x, int li, int g, int cap) {
  WsView L = ws_view(p, li, g);
  const int l = p.first + li;
  L.cap = cap; L.P = cap + 1;
  double* w = p.work + x.est_base + (int64_t)p.G * (x.est_pre[l] - x.est_pre[p.first]) + (int64_t)g * (x.est_pre[l + 1] - x.est_pre[l]);
  L.Am = w; L.Bm = L.Am + (int64_t)L.S * L.P; L.Em = L.Bm + (int64_t)L.S * L.P; L.gamma = L.Em + (int64_t)L.S * L.P;
  L.part = L.gamma + (int64_t)L.W * L.P;
  L.topv = nullptr; L.topw = nullptr;
  return L;
}

__device__ __forceinline__ void wc_no_result(const WsParams& p, const WcParams& x, int pair, int status, int system) {
  p.nwords[pair] = 0; p.risk[pair] = 0.0; p.iterations[pair] = 0; p.status[pair] = status; x.system[pair] = system;
  if (p.bin_n) p.bin_n[pair] = 0;
}

__global__ void __launch_bounds__(kWsThreads) wc_init_kernel(WsParams p, WcParams x) {
  __shared__ int32_t sel[2];
  const int pair = blockIdx.x, gl = pair / p.G, g = pair % p.G, gi = x.g0 + gl, tid = threadIdx.x;
  const WcGroup U = wc_group(p, x, gi, g);
  if (tid == 0) {
    int ks = -1, st = 0;
    double bs = 0.0;
    for (int k = 0; k < U.K; ++k) {
      const int l = U.l0 + k;
      const WsView L = ws_view(p, l - p.first, g);
      if (L.best[0] < 0) { st = 3; break; }        // no finite alpha(end): the group fails
      const double s = (L.v[L.S - 1] + L.alpha[L.S - 1]) - x.logwn[l];
      if (ks < 0 || s < bs) { ks = k; bs = s; }      // a later system wins only on <
    }
    sel[0] = st == 3 ? -1 : ks; sel[1] = st;
  }
  __syncthreads();
  const int ks = sel[0];
  if (ks < 0) {
    if (tid == 0) { wc_no_result(p, x, pair, 3, -1); U.hd[0] = 0; U.hd[1] = 0; U.hd[2] = 1; U.hd[3] = -1; }
    return;
  }
  const WsView L = ws_view(p, U.l0 + ks - p.first, g);
  const int m0 = L.best[0];
  if (2 * m0 + 1 > U.cap) {                          // a first hypothesis beyond the row capacity
    if (tid == 0) { wc_no_result(p, x, pair, 2, ks); U.hd[0] = 0; U.hd[1] = 0; U.hd[2] = 1; U.hd[3] = ks; }
    return;
  }
  U.R[tid] = 0;
  __syncthreads();
  if (tid < m0) {
    const int gid = L.word_ids[L.best[1 + tid]];
    int lo = 0, hi = U.WU - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (U.uvoc[mid] < gid) lo = mid + 1; else hi = mid; }
    U.R[2 * (tid + 1)] = lo;
  }
  if (tid == 0) { U.hd[0] = 2 * m0 + 1; U.hd[1] = 0; U.hd[2] = 0; U.hd[3] = ks; }
}

__global__ void __launch_bounds__(kWsThreads) wc_estep_kernel(WsParams p, WcParams x) {
  __shared__ int32_t r[kWsThreads];
  __shared__ unsigned char decs[kWsWaves * kWsThreads];
  __shared__ double epart[kWsWaves][64];
  const int pair = blockIdx.x, li = pair / p.G, g = pair % p.G, l = p.first + li, gi = x.lat_group[l], tid = threadIdx.x;
  const WcGroup U = wc_group(p, x, gi, g);
  if (U.hd[2]) return;
  const WsView L = wc_view(p, x, li, g, U.cap);
  const int Q = U.hd[0];
  const int32_t* map = x.map + x.map_off[l];
  const int ru = tid <= Q ? U.R[tid] : 0;            // ru < WU: the update kernel's argmax, or the init kernel's search
  r[tid] = ru != 0 ? map[ru] : 0;                    // W_k for a word the system does not have: no arc carries it
  __syncthreads();
  ws_estep(L, r, Q, decs, epart);
}

__global__ void __launch_bounds__(kWsThreads) wc_update_kernel(WsParams p, WcParams x) {
  __shared__ int32_t r[kWsThreads];
  __shared__ int32_t best[kWsThreads];
  __shared__ int32_t wave_tot[kWsWaves];
  __shared__ const double* s_gamma[kWcMaxSystems];
  __shared__ const int32_t* s_map[kWcMaxSystems];
  __shared__ double s_wn[kWcMaxSystems], s_risk[kWcMaxSystems];
  __shared__ int32_t s_W[kWcMaxSystems];
  const int pair = blockIdx.x, gl = pair / p.G, g = pair % p.G, gi = x.g0 + gl, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WcGroup U = wc_group(p, x, gi, g);
  if (U.hd[2]) return;
  const int Q = U.hd[0], P = U.P, kk = p.kk, K = U.K, WU = U.WU;
  r[tid] = tid <= Q ? U.R[tid] : 0;
  if (tid < K) {
    const int l = U.l0 + tid;
    const WsView L = wc_view(p, x, l - p.first, g, U.cap);
    s_gamma[tid] = L.gamma; s_map[tid] = x.map + x.map_off[l]; s_wn[tid] = x.wn[l]; s_W[tid] = L.W;
    s_risk[tid] = L.Am[(int64_t)(L.S - 1) * P + Q];
  }
  __syncthreads();
  // ---- Gamma(q)[w] = sum over the systems that have w, in ascending k, of wn_k gamma_k(q)[loc_k(w)] ----
  for (int64_t i = tid; i < (int64_t)WU * (Q + 1); i += kWsThreads) {
    const int w = (int)(i / (Q + 1)), q = (int)(i - (int64_t)w * (Q + 1));
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const int loc = s_map[k][w];
      if (loc < s_W[k]) acc += s_wn[k] * s_gamma[k][(int64_t)loc * P + q];
    }
    U.Gamma[(int64_t)w * P + q] = acc;
  }
  __syncthreads();
  ws_top_entries(U.Gamma, WU, P, Q, kk, U.topv, U.topw, best);
  __syncthreads();
  // ---- decision: thread q looks at position q (as ws_mbr_kernel) ----
  const int iter = U.hd[1] + 1;
  const bool in = tid >= 1 && tid <= Q;
  const int nb = in ? best[tid] : 0;
  const bool flag = in && nb > 0;
  const int changed = __syncthreads_or(in && nb != r[tid]);
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) wave_tot[wave] = __popcll(mask);
  __syncthreads();
  int idx = __popcll(mask & ((1ull << lane) - 1ull)), mnew = 0;
  for (int w2 = 0; w2 < kWsWaves; ++w2) { const int t2 = wave_tot[w2]; if (w2 < wave) idx += t2; mnew += t2; }
  int status = -1;
  if (!p.decode_mbr || !changed) status = 0;
  else if (iter >= p.max_iter) status = 1;
  else if (2 * mnew + 1 > U.cap) status = 2;
  if (status < 0) {                                  // another round: the new hypothesis
    U.R[tid] = 0;
    __syncthreads();
    if (flag) U.R[2 * (idx + 1)] = nb;
    if (tid == 0) { U.hd[0] = 2 * mnew + 1; U.hd[1] = iter; }
    return;
  }
  // ---- result: the hypothesis of this E-step with its own statistics ----
  const int m = (Q - 1) / 2;
  if (tid < m && tid < p.word_stride) {
    const int w = r[2 * (tid + 1)];
    p.words[(int64_t)pair * p.word_stride + tid] = U.uvoc[w];
    p.conf[(int64_t)pair * p.word_stride + tid] = U.Gamma[(int64_t)w * P + 2 * (tid + 1)];
  }
  if (p.bins > 0 && flag && idx < p.bin_stride) {
    for (int t = 0; t < p.bins; ++t) {
      const int w = U.topw[(int64_t)tid * kk + t];
      const int64_t o = ((int64_t)pair * p.bin_stride + idx) * p.bins + t;
      p.bin_word[o] = w >= 0 ? U.uvoc[w] : -1;
      p.bin_post[o] = w >= 0 ? U.topv[(int64_t)tid * kk + t] : 0.0;
    }
  }
  if (tid == 0) {
    double risk = 0.0;
    for (int k = 0; k < K; ++k) risk += s_wn[k] * s_risk[k];
    p.nwords[pair] = m; p.risk[pair] = risk; p.iterations[pair] = iter; p.status[pair] = status; x.system[pair] = U.hd[3];
    if (p.bin_n) p.bin_n[pair] = mnew;
    U.hd[1] = iter; U.hd[2] = 1;
  }
}

// ---- host ----
bool wc_range_ok(const WordLat* h, int g0, int gcount) {
  return h && h->NG >= 1 && g0 >= 0 && gcount >= 1 && (int64_t)g0 + gcount <= h->NG;
}

// words of workspace: [post of the lattices | E-step rows of the lattices | the groups' areas], each times G
void wc_words(const WordLat* h, int g0, int gcount, int G, int bins, int64_t& post, int64_t& est, int64_t& grp) {
  const int f = h->group_off[g0], e = h->group_off[g0 + gcount];
  const int64_t kk = bins > 1 ? bins : 1;
  post = (h->post_pre[e] - h->post_pre[f]) * G;
  est = (h->est_pre[e] - h->est_pre[f]) * G;
  grp = ((h->grp_pre[g0 + gcount] - h->grp_pre[g0]) + 3 * kk * (h->gpe_pre[g0 + gcount] - h->gpe_pre[g0]) / 2) * G;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" int pk2_wordlat_set_groups(void* handle, int32_t NG, const int32_t* group_off, const double* wn, const double* log_wn,
                                      const int64_t* uvoc_off, const int32_t* uvoc, const int32_t* map) {
  WordLat* h = static_cast<WordLat*>(handle);
  PK2_REQUIRE(h && group_off && wn && log_wn && uvoc_off && uvoc && map, "wordlat_set_groups: null pointer");
  PK2_REQUIRE(h->N >= 1 && NG >= 1 && NG <= h->N, "wordlat_set_groups: %d groups for %d lattices", NG, h->N);
  PK2_REQUIRE(group_off[0] == 0 && group_off[NG] == h->N && uvoc_off[0] == 0, "wordlat_set_groups: the groups must cover the batch");
  const int N = h->N;
  std::vector<int32_t> lat_group(N), gcap(NG);
  std::vector<int64_t> map_off(N + 1, 0), est_pre(N + 1, 0), grp_pre(NG + 1, 0), gpe_pre(NG + 1, 0);
  for (int gi = 0; gi < NG; ++gi) {
    const int l0 = group_off[gi], K = group_off[gi + 1] - l0;
    PK2_REQUIRE(K >= 1 && K <= kWcMaxSystems, "wordlat_set_groups: group %d holds %d systems (1..%d)", gi, K, kWcMaxSystems);
    const int64_t WU = uvoc_off[gi + 1] - uvoc_off[gi];
    PK2_REQUIRE(WU >= 1 && WU < (1 << 30), "wordlat_set_groups: group %d has a vocabulary of %lld words", gi, (long long)WU);
    const int32_t* uv = uvoc + uvoc_off[gi];
    PK2_REQUIRE(uv[0] == 0, "wordlat_set_groups: the vocabulary of group %d does not start with 0", gi);
    for (int64_t w = 1; w < WU; ++w)
      PK2_REQUIRE(uv[w] > uv[w - 1], "wordlat_set_groups: the vocabulary of group %d is not ascending", gi);
    double sum = 0.0;
    int depth = 0;
    for (int l = l0; l < l0 + K; ++l) {
      PK2_REQUIRE(std::isfinite(wn[l]) && wn[l] > 0.0 && wn[l] <= 1.0 && std::isfinite(log_wn[l]) &&
                  std::fabs(log_wn[l] - std::log(wn[l])) <= 1e-12, "wordlat_set_groups: weight %g (log %g) of lattice %d", wn[l],
                  log_wn[l], l);
      sum += wn[l];
      depth = std::max(depth, h->depth[l]);
    }
    PK2_REQUIRE(std::fabs(sum - 1.0) <= 1e-12, "wordlat_set_groups: the weights of group %d add up to %.17g", gi, sum);
    const int64_t cap = std::min<int64_t>(PK2_WORDLAT_MAX_POSITIONS, 2 * (int64_t)depth + 1), P = cap + 1;
    gcap[gi] = (int32_t)cap;
    for (int l = l0; l < l0 + K; ++l) {
      // the map of a system: union local id -> system local id, W_l for a word it does not have; every word of the
      // system must be reached (both id lists ascend, so equal ids at ascending positions make the map consistent)
      const int64_t W = h->word_off_off[l + 1] - h->word_off_off[l] - 1;
      const int32_t* wi = h->h_word_ids.data() + h->word_off_off[l] - l;
      const int32_t* mp = map + map_off[l];
      int64_t have = 0;
      for (int64_t w = 0; w < WU; ++w) {
        PK2_REQUIRE(mp[w] >= 0 && mp[w] <= W && (mp[w] == W || wi[mp[w]] == uv[w]),
                    "wordlat_set_groups: lattice %d, entry %lld of its word map", l, (long long)w);
        have += mp[w] < W;
      }
      PK2_REQUIRE(have == W && mp[0] == 0, "wordlat_set_groups: the vocabulary of group %d lacks words of lattice %d", gi, l);
      lat_group[l] = gi;
      map_off[l + 1] = map_off[l] + WU;
      est_pre[l + 1] = est_pre[l] + ws_mbr_words(h->state_off[l + 1] - h->state_off[l], W, P);
    }
    grp_pre[gi + 1] = grp_pre[gi] + WU * P + kWcStateWords;
    gpe_pre[gi + 1] = gpe_pre[gi] + ((P + 1) & ~(int64_t)1);
  }
  const size_t TU = (size_t)uvoc_off[NG], TM = (size_t)map_off[N];
  auto carve = [&](Carver& c, WordLat* o) {
    o->d_group_off = c.take<int32_t>(NG + 1); o->d_lat_group = c.take<int32_t>(N); o->d_gcap = c.take<int32_t>(NG);
    o->d_uvoc = c.take<int32_t>(TU); o->d_map = c.take<int32_t>(TM); o->d_wn = c.take<double>(N); o->d_logwn = c.take<double>(N);
    o->d_uvoc_off = c.take<int64_t>(NG + 1); o->d_map_off = c.take<int64_t>(N + 1); o->d_est_pre = c.take<int64_t>(N + 1);
    o->d_grp_pre = c.take<int64_t>(NG + 1); o->d_gpe_pre = c.take<int64_t>(NG + 1);
  };
  Carver sz(nullptr);
  WordLat dummy;
  carve(sz, &dummy);
  if (h->gblob) { PK2_HIP(hipFree(h->gblob)); h->gblob = nullptr; h->NG = 0; }
  PK2_HIP(hipMalloc(&h->gblob, sz.bytes()));
  Carver cv(h->gblob);
  carve(cv, h);
  auto up = [&](const void* d, const void* s, size_t n) { return hipMemcpy(const_cast<void*>(d), s, n, hipMemcpyHostToDevice); };
  PK2_HIP(up(h->d_group_off, group_off, 4 * (NG + 1))); PK2_HIP(up(h->d_lat_group, lat_group.data(), 4 * N));
  PK2_HIP(up(h->d_gcap, gcap.data(), 4 * NG)); PK2_HIP(up(h->d_uvoc, uvoc, 4 * TU)); PK2_HIP(up(h->d_map, map, 4 * TM));
  PK2_HIP(up(h->d_wn, wn, 8 * N)); PK2_HIP(up(h->d_logwn, log_wn, 8 * N)); PK2_HIP(up(h->d_uvoc_off, uvoc_off, 8 * (NG + 1)));
  PK2_HIP(up(h->d_map_off, map_off.data(), 8 * (N + 1))); PK2_HIP(up(h->d_est_pre, est_pre.data(), 8 * (N + 1)));
  PK2_HIP(up(h->d_grp_pre, grp_pre.data(), 8 * (NG + 1))); PK2_HIP(up(h->d_gpe_pre, gpe_pre.data(), 8 * (NG + 1)));
  h->group_off.assign(group_off, group_off + NG + 1);
  h->gcap = gcap; h->est_pre = est_pre; h->grp_pre = grp_pre; h->gpe_pre = gpe_pre;
  h->NG = NG;
  return PK2_OK;
}

extern "C" size_t pk2_wordlat_combine_workspace_bytes(const void* handle, int32_t first_group, int32_t group_count, int32_t G,
                                                      int32_t bins) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  if (!wc_range_ok(h, first_group, group_count) || G < 1 || G > PK2_WORDLAT_MAX_SETTINGS || bins < 0 || bins > PK2_WORDLAT_MAX_BINS)
    return 0;
  int64_t post, est, grp;
  wc_words(h, first_group, group_count, G, bins, post, est, grp);
  return (size_t)(post + est + grp) * 8;
}

extern "C" int pk2_wordlat_combine(const void* handle, int32_t first_group, int32_t group_count, const double* settings,
                                   int32_t G, int32_t decode_mbr, int32_t max_iter, int32_t bins, void* work, size_t work_bytes,
                                   int32_t* words, double* conf, int32_t word_stride, int32_t* nwords, double* risk,
                                   int32_t* iterations, int32_t* status, int32_t* system, int32_t* bin_n, int32_t* bin_word,
                                   double* bin_post, int32_t bin_stride, void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && settings && work && words && conf && nwords && risk && iterations && status && system,
              "wordlat_combine: null pointer");
  PK2_REQUIRE(h->NG >= 1, "wordlat_combine: no groups (pk2_wordlat_set_groups comes first)");
  PK2_REQUIRE(G >= 1 && G <= PK2_WORDLAT_MAX_SETTINGS, "wordlat_combine: %d settings (1..%d)", G, PK2_WORDLAT_MAX_SETTINGS);
  PK2_REQUIRE(bins >= 0 && bins <= PK2_WORDLAT_MAX_BINS, "wordlat_combine: bins %d (0..%d)", bins, PK2_WORDLAT_MAX_BINS);
  PK2_REQUIRE(bins == 0 || (bin_n && bin_word && bin_post), "wordlat_combine: null pointer for the bins");
  PK2_REQUIRE(max_iter >= 1 && max_iter <= PK2_WORDLAT_COMBINE_MAX_ITER, "wordlat_combine: max_iter %d (1..%d)", max_iter,
              PK2_WORDLAT_COMBINE_MAX_ITER);
  PK2_REQUIRE(ws_settings_ok(settings, G), "wordlat_combine: non-finite scale");
  PK2_REQUIRE(wc_range_ok(h, first_group, group_count), "wordlat_combine: groups %d..%d of %d", first_group,
              first_group + group_count, h->NG);
  for (int gi = first_group; gi < first_group + group_count; ++gi) {
    PK2_REQUIRE(word_stride >= (h->gcap[gi] - 1) / 2, "wordlat_combine: word_stride %d, group %d can hold %d words", word_stride, gi,
                (h->gcap[gi] - 1) / 2);
    PK2_REQUIRE(bins == 0 || bin_stride >= h->gcap[gi], "wordlat_combine: bin_stride %d below the capacity %d of group %d",
                bin_stride, h->gcap[gi], gi);
  }
  int64_t post, est, grp;
  wc_words(h, first_group, group_count, G, bins, post, est, grp);
  PK2_REQUIRE(work_bytes >= (size_t)(post + est + grp) * 8 && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_combine: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, (size_t)(post + est + grp) * 8);
  const int first = h->group_off[first_group], count = h->group_off[first_group + group_count] - first;
  hipStream_t st = static_cast<hipStream_t>(stream);
  WsParams p;
  ws_fill(h, p, first, count, settings, G, false, bins);
  p.work = static_cast<double*>(work);
  p.decode_mbr = decode_mbr != 0; p.max_iter = max_iter;
  p.words = words; p.conf = conf; p.word_stride = word_stride; p.nwords = nwords; p.risk = risk; p.iterations = iterations;
  p.status = status; p.bin_n = bins ? bin_n : nullptr; p.bin_word = bin_word; p.bin_post = bin_post; p.bin_stride = bin_stride;
  WcParams x;
  x.group_off = h->d_group_off; x.lat_group = h->d_lat_group; x.gcap = h->d_gcap; x.uvoc = h->d_uvoc; x.map = h->d_map;
  x.wn = h->d_wn; x.logwn = h->d_logwn; x.uvoc_off = h->d_uvoc_off; x.map_off = h->d_map_off; x.est_pre = h->d_est_pre;
  x.grp_pre = h->d_grp_pre; x.gpe_pre = h->d_gpe_pre; x.g0 = first_group; x.gcount = group_count;
  x.est_base = post; x.grp_base = post + est; x.system = system;
  const int rc = ws_launch_post(h, first, count, settings, G, p.work, st);
  if (rc != PK2_OK) return rc;
  hipLaunchKernelGGL(wc_init_kernel, dim3(group_count * G), dim3(kWsThreads), 0, st, p, x);
  PK2_LAUNCH_CHECK();
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(wc_estep_kernel, dim3(count * G), dim3(kWsThreads), 0, st, p, x);
    PK2_LAUNCH_CHECK();
    hipLaunchKernelGGL(wc_update_kernel, dim3(group_count * G), dim3(kWsThreads), 0, st, p, x);
    PK2_LAUNCH_CHECK();
  }
  return PK2_OK;
}
