// N-best paths of the device lattices and the N-best minimum word error criterion (MWEFunction) on gfx950.
//
// Replaces, per minibatch and on the device (reference ops/ops.py:158-241):
//   scale_lattice(lattice_scale(lm_weight, am_weight)); [convert_lattice_to_phones]; convert_lattice_to_std;
//   nbest_as_fsts(num_paths); get_linear_symbol_sequence; editdistance.eval; softmax(-weights); grad scatter.
// The lattice never leaves HBM.  The arithmetic and the tie rule are restated in tests/mwe_ref.py:
//   * link cost = float(float(lm * graph) + float(am * acoustic)) (products in double), path cost = float32 sum of the
//     link costs in path order from the start, plus float(lm * final) last; no floating-point contraction;
//   * equal costs are ordered by the back-pointer's content: (source frame, source HCLG state), transition-id, graph cost
//     bits, source rank; the final selection by (final token's HCLG state, rank).  Never by the order of the links in the
//     workspace, which the decoder appends with atomics.
//
// Kernels (one launch each, in stream order):
//   nb_prep      per-utterance offsets of the scratch lists (prefix sums of the decoder's token / link counts)
//   nb_labels    the output label of every kept link: word (HCLG arc search, as pk2_decode_graph_link_words) or phone
//   nb_kbest     one workgroup per utterance: per token the K best (or K best distinct-label) partial paths, frame by
//                frame; a frame's kept links are grouped by destination (LDS, or global memory for large frames) and one
//                wavefront merges a destination's candidates, destinations in epsilon-level order; then the final merge
//   nb_backtrace one lane per path: transition-id per frame, labels, and (reference mode) the drop of repeated labels
//   mwe_edit     one wavefront per (utterance, hypothesis): Levenshtein distance to the supervision
//   mwe_loss     p_k, loss (float64), g_k = (e_k - loss) p_k
//   mwe_grad     one thread per (utterance, frame): grad[t, pdf] = sum of g_k in hypothesis order, no atomics
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "lattice_edit.h"
#include "lattice_internal.h"
#include "persist_guard.h"

#pragma clang fp contract(off)

namespace pk2 {

constexpr int kNbThreads = 1024;
constexpr int kNbWaves = kNbThreads / 64;
constexpr int kNbSlots = 4;            // candidate slots per lane of a merge pass: 256 per wavefront
constexpr int kNbMaxPaths = 64;
constexpr int kNbLds = 150 * 1024;     // LDS of nb_kbest: merge lists, then the grouping of a frame's links
constexpr uint64_t kNbHash0 = 1469598103934665603ull;

__host__ __device__ __forceinline__ uint64_t nb_hash_step(uint64_t h, int32_t label) {
  if (label == 0) return h;
  uint64_t z = h ^ ((uint64_t)(uint32_t)label + 0x9E3779B97F4A7C15ull);
  z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 31;
  z *= 0x94D049BB133111EBull; z ^= z >> 29;
  return z;
}
__device__ __forceinline__ uint32_t nb_enc(float c) {
  const uint32_t b = __float_as_uint(c);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct NbParams {
  LatPtrs L;
  int32_t N, Tmax, K, distinct, label_cap, cap, lcap;
  double lm, am;
  int64_t tok_total, link_total;
  // labels
  int32_t label_mode;          // 0 words, 1 phones
  const int32_t* tid2label; int32_t num_tids;
  DevDecodeGraph G; const int32_t* e_ol; const int32_t* n_ol; const int32_t* e_perm; const int32_t* n_perm;
  // scratch
  int64_t* tok_off; int64_t* link_off; int32_t* ok;
  float* e_cost; int2* e_bp; uint64_t* e_hash; int32_t* e_n;
  int32_t* lab; int32_t* gC; int32_t* gI; int32_t* gAd; int32_t* gAn;
  float* f_cost; int2* f_bp; uint64_t* f_hash; int32_t* f_n;
  // paths: [N, K] (labels [N, K, label_cap], tids [N, K, Tmax])
  int32_t* num_hyp; int32_t* hyp_path; float* path_cost; int32_t* path_nlab; int32_t* path_labels; int32_t* path_tids;
  uint64_t* path_hash;
};

__global__ void nb_prep(NbParams p) {
  if (threadIdx.x != 0) return;
  int64_t t = 0, l = 0;
  for (int n = 0; n < p.N; ++n) {
    const LatUtt U = p.L.utt[n];
    p.tok_off[n] = t; p.link_off[n] = l;
    const bool fits = U.status == kLatOk && t + U.n_tok <= p.tok_total && l + U.n_link <= p.link_total;
    p.ok[n] = fits ? 1 : 0;
    if (fits) { t += U.n_tok; l += U.n_link; }
  }
}

// Label of every kept link.  Words: the arc of the link's HCLG source state with the same destination and transition-id
// (epsilon arcs for transition-id 0) whose weight is nearest the link's graph cost, first one on a tie; -1 when none.
__global__ void nb_labels(NbParams p) {
  const int n = blockIdx.y, s = blockIdx.x;
  if (!p.ok[n]) return;
  const LatUtt U = p.L.utt[n];
  if (s >= 2 * (U.T + 1)) return;
  const int32_t* seg = p.L.seg_off + U.frame_base;
  const int l0 = seg[s], l1 = l0 + p.L.seg_kept[U.frame_base + s];
  const int4* lrec = p.L.link_rec + U.link_base;
  const int32_t* st = p.L.tok_state + U.tok_base;
  int32_t* lab = p.lab + p.link_off[n];
  for (int l = l0 + (int)threadIdx.x; l < l1; l += blockDim.x) {
    if (l < 0 || l >= U.n_link) continue;
    const int4 r = lrec[l];
    int32_t out = 0;
    if (p.label_mode == 1) {
      out = (r.z > 0 && r.z <= p.num_tids) ? p.tid2label[r.z] : 0;
    } else if ((unsigned)r.x < (unsigned)U.n_tok && (unsigned)r.y < (unsigned)U.n_tok) {
      const int32_t a = st[r.x], d = st[r.y];
      const float g = __int_as_float(r.w);
      float bd = INFINITY;
      out = -1;
      if (a >= 0 && a < p.G.S) {
        // the state's arcs in (destination, transition-id, arc) order: the first one with this destination, by bisection
        // (the word-loop state has an epsilon arc per word)
        const bool em = r.z > 0;
        const int32_t* perm = em ? p.e_perm : p.n_perm;
        const int32_t* adst = em ? p.G.e_dst : p.G.n_dst;
        const float* aw = em ? p.G.e_w : p.G.n_w;
        const int32_t* aol = em ? p.e_ol : p.n_ol;
        int lo = em ? p.G.e_off[a] : p.G.n_off[a], hi = em ? p.G.e_off[a + 1] : p.G.n_off[a + 1];
        const int end = hi;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1, k = perm[mid];
          const bool less = adst[k] < d || (adst[k] == d && em && p.G.e_tid[k] < r.z);
          if (less) lo = mid + 1; else hi = mid;
        }
        for (int i = lo; i < end; ++i) {
          const int k = perm[i];
          if (adst[k] != d || (em && p.G.e_tid[k] != r.z)) break;
          const float dd = fabsf(aw[k] - g);
          if (dd < bd) { bd = dd; out = aol[k]; }
        }
      }
    }
    lab[l] = out;
  }
}

// One list entry while a wavefront merges (LDS).  bp = kept link (final merge: final token), rank = source entry.
struct NbE { float cost; uint32_t fs; uint32_t tid; uint32_t gb; int32_t rank; int32_t bp; uint64_t hash; };
// Sort key: a = (cost, source frame bit | source state), b = (transition-id, graph cost bits), c = (rank, slot)
struct NbKey { uint64_t a, b; uint32_t c; };
__device__ __forceinline__ bool nb_less(const NbKey& x, const NbKey& y) {
  return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.c < y.c);
}
__device__ __forceinline__ NbKey nb_wave_min(NbKey k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    NbKey q{__shfl_xor(k.a, o, 64), __shfl_xor(k.b, o, 64), __shfl_xor(k.c, o, 64)};
    if (nb_less(q, k)) k = q;
  }
  return k;
}
__device__ __forceinline__ void nb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A candidate source of a merge: the partial paths of token `src` extended by a link (or, in the final merge, by the
// final cost).  src < 0: none.
struct NbItem { int src; float add; uint32_t fs, tid, gb; int32_t label, bp; };

// One wavefront merges the candidates of `nitems` items into the sorted list of at most K entries of one destination.
// The candidates of up to 256 / K items are loaded at a time (slot q = item * K + rank); the K smallest of them are
// selected by K rounds of a wavefront minimum and merged with the list so far (acc, sorted, in LDS).
template <class ItemFn>
__device__ void nb_merge(const NbParams& p, const float* ec, const uint64_t* eh, const int32_t* en, int nitems, ItemFn item,
                         NbE* acc, NbE* out, float* d_cost, int2* d_bp, uint64_t* d_hash, int32_t* d_n) {
  const int K = p.K, lane = threadIdx.x & 63;
  const int CL = max(1, (64 * kNbSlots) / K);
  const NbKey none{~0ull, ~0ull, ~0u};
  int nacc = 0;
  for (int j0 = 0; j0 < nitems; j0 += CL) {
    const int cl = min(CL, nitems - j0);
    NbKey key[kNbSlots]; float cst[kNbSlots]; int32_t bpv[kNbSlots]; uint64_t hs[kNbSlots];
#pragma unroll
    for (int i = 0; i < kNbSlots; ++i) {
      const int q = lane + 64 * i;
      key[i] = none; cst[i] = 0.f; bpv[i] = 0; hs[i] = 0;
      if (q < cl * K) {
        const int r = q % K;
        const NbItem it = item(j0 + q / K);
        if (it.src >= 0 && r < en[it.src]) {
          const int64_t e = (int64_t)it.src * K + r;
          const float c = __fadd_rn(ec[e], it.add);
          key[i] = NbKey{((uint64_t)nb_enc(c) << 32) | it.fs, ((uint64_t)it.tid << 32) | it.gb, ((uint32_t)r << 16) | (uint32_t)q};
          cst[i] = c; bpv[i] = it.bp;
          hs[i] = p.distinct ? nb_hash_step(eh[e], it.label) : 0;
        }
      }
    }
    int a = 0, nout = 0;
    uint64_t oh = 0;          // lane r: hash of out[r]
    while (nout < K) {
      NbKey best = none;
#pragma unroll
      for (int i = 0; i < kNbSlots; ++i) if (nb_less(key[i], best)) best = key[i];
      const NbKey wb = nb_wave_min(best);
      const bool have = wb.a != ~0ull;
      bool use_acc = false;
      NbE e;
      if (a < nacc) {
        e = acc[a];
        const NbKey ka{((uint64_t)nb_enc(e.cost) << 32) | e.fs, ((uint64_t)e.tid << 32) | e.gb, (uint32_t)e.rank << 16};
        const NbKey wq{wb.a, wb.b, wb.c & 0xFFFF0000u};
        use_acc = !have || !nb_less(wq, ka);
      }
      if (!have && !use_acc) break;
      if (use_acc) {
        ++a;
      } else {
        const int q = (int)(wb.c & 0xFFFFu), owner = q & 63, slot = q >> 6;
        float mc = 0.f; int32_t mb = 0; uint64_t mh = 0;
#pragma unroll
        for (int i = 0; i < kNbSlots; ++i)
          if (i == slot) { mc = cst[i]; mb = bpv[i]; mh = hs[i]; if (lane == owner) key[i] = none; }
        e.cost = __shfl(mc, owner, 64); e.bp = __shfl(mb, owner, 64); e.hash = __shfl(mh, owner, 64);
        e.fs = (uint32_t)wb.a; e.tid = (uint32_t)(wb.b >> 32); e.gb = (uint32_t)wb.b; e.rank = (int32_t)(wb.c >> 16);
      }
      if (p.distinct && __ballot(lane < nout && oh == e.hash)) continue;
      if (lane == 0) out[nout] = e;
      if (lane == nout) oh = e.hash;
      ++nout;
    }
    nb_wave_sync();
    NbE* t = acc; acc = out; out = t; nacc = nout;
  }
  for (int r = lane; r < nacc; r += 64) {
    const NbE e = acc[r];
    d_cost[r] = e.cost; d_bp[r] = make_int2(e.bp, e.rank);
    if (p.distinct) d_hash[r] = e.hash;
  }
  if (lane == 0) *d_n = nacc;
  nb_wave_sync();
}

// Exclusive prefix sum of a[0..n) by the whole workgroup (a in LDS or global memory).
__device__ void nb_block_scan(int32_t* a, int n, int32_t* red) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0;
  for (int b0 = 0; b0 < n; b0 += kNbThreads) {
    const int i = b0 + tid;
    const int v = i < n ? a[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) red[w] = x;
    __syncthreads();
    int off = carry, tot = 0;
    for (int k = 0; k < kNbWaves; ++k) { if (k < w) off += red[k]; tot += red[k]; }
    if (i < n) a[i] = off + x - v;
    carry += tot;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kNbThreads) nb_kbest(NbParams p) {
  extern __shared__ __attribute__((aligned(16))) NbE nb_smem[];
  __shared__ int32_t red[kNbWaves];
  const int n = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  if (!p.ok[n]) return;
  const LatUtt U = p.L.utt[n];
  const int K = p.K, T = U.T;
  const int32_t* ftok = p.L.frame_tok + U.frame_base;
  const int32_t* seg = p.L.seg_off + U.frame_base;
  const int32_t* kept = p.L.seg_kept + U.frame_base;
  const int32_t* maxlev = p.L.frame_maxlev + U.frame_base;
  const int4* lrec = p.L.link_rec + U.link_base;
  const float* lac = p.L.link_ac + U.link_base;
  const int32_t* tl = p.L.tok_level + U.tok_base;
  const float* tf = p.L.tok_final + U.tok_base;
  const int32_t* tst = p.L.tok_state + U.tok_base;
  const int64_t toff = p.tok_off[n], loff = p.link_off[n];
  float* ec = p.e_cost + toff * K; int2* eb = p.e_bp + toff * K;
  uint64_t* eh = p.distinct ? p.e_hash + toff * K : nullptr;
  int32_t* en = p.e_n + toff;
  const int32_t* lab = p.lab + loff;
  NbE* acc = nb_smem + (size_t)w * 2 * K;
  NbE* out = acc + K;
  int32_t* sC = reinterpret_cast<int32_t*>(nb_smem + (size_t)kNbWaves * 2 * K);
  int32_t* sI = sC + p.cap;
  int32_t* sAd = sI + p.lcap;
  int32_t* sAn = sAd + p.lcap;
  __shared__ int32_t nact_s;
  const int ntok = U.n_tok, nlink = U.n_link;
  if (tid == 0) {        // the start token: frame 0, local token 0, the empty path
    en[0] = 1; ec[0] = 0.f; eb[0] = make_int2(-1, 0);
    if (eh) eh[0] = kNbHash0;
  }
  __syncthreads();
  for (int t = 0; t <= T; ++t) {
    const int base = ftok[t], cnt = ftok[t + 1] - base;
    const int m0 = t > 0 ? seg[2 * t - 1] : 0, nm = t > 0 ? kept[2 * t - 1] : 0;
    const int e0 = seg[2 * t], ne = kept[2 * t], nl = nm + ne;
    // the frame's tokens: Cc (links into each); its destinations (tokens with a kept link into them): Ad / An (token,
    // link count, then first link); Ii: the links grouped by destination
    const bool lds = cnt <= p.cap && nl <= p.lcap;
    const int64_t lo = loff + (t > 0 ? m0 : e0);
    int32_t* Cc = lds ? sC : p.gC + toff + (int64_t)n * (p.Tmax + 2) + base + t;
    int32_t* Ii = lds ? sI : p.gI + lo;
    int32_t* Ad = lds ? sAd : p.gAd + lo;
    int32_t* An = lds ? sAn : p.gAn + lo;
    auto link_of = [&](int q) { return q < nm ? m0 + q : e0 + (q - nm); };
    for (int i = tid; i < cnt; i += kNbThreads) Cc[i] = 0;
    if (tid == 0) nact_s = 0;
    __syncthreads();
    for (int q = tid; q < nl; q += kNbThreads) {
      const int d = lrec[link_of(q)].y - base;
      if (d >= 0 && d < cnt) atomicAdd(&Cc[d], 1);
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += kNbThreads) {
      const int c = Cc[i];
      if (c > 0) { const int k = atomicAdd(&nact_s, 1); Ad[k] = i; An[k] = c; }
      else if (!(t == 0 && i == 0) && base + i < ntok) en[base + i] = 0;     // (a token nobody reaches: empty list)
    }
    __syncthreads();
    const int nact = nact_s;
    nb_block_scan(An, nact, red);
    for (int k = tid; k < nact; k += kNbThreads) Cc[Ad[k]] = An[k];
    __syncthreads();
    for (int q = tid; q < nl; q += kNbThreads) {
      const int l = link_of(q);
      const int d = lrec[l].y - base;
      if (d >= 0 && d < cnt) Ii[atomicAdd(&Cc[d], 1)] = l;
    }
    __syncthreads();
    const int nlev = max(0, maxlev[t]);
    for (int lev = 0; lev <= nlev; ++lev) {
      for (int k = w; k < nact; k += kNbWaves) {
        const int d = Ad[k], g = base + d;
        if ((t == 0 && d == 0) || g >= ntok) continue;
        if (nlev > 0 && min(max(tl[g], 0), nlev) != lev) continue;
        const int s0 = An[k], s1 = Cc[d];
        auto item = [&](int j) -> NbItem {
          NbItem it{-1, 0.f, 0, 0, 0, 0, 0};
          const int l = Ii[s0 + j];
          if (l < 0 || l >= nlink) return it;
          const int4 r = lrec[l];
          if ((unsigned)r.x >= (unsigned)ntok) return it;
          it.src = r.x;
          it.add = __fadd_rn((float)(p.lm * (double)__int_as_float(r.w)), (float)(p.am * (double)lac[l]));
          it.fs = ((r.x >= base ? 1u : 0u) << 31) | (uint32_t)tst[r.x];
          it.tid = (uint32_t)r.z; it.gb = (uint32_t)r.w; it.label = lab[l]; it.bp = l;
          return it;
        };
        nb_merge(p, ec, eh, en, s1 - s0, item, acc, out, ec + (int64_t)g * K, eb + (int64_t)g * K,
                 eh ? eh + (int64_t)g * K : nullptr, en + g);
      }
      __syncthreads();
    }
  }
  // final merge: the last frame's final tokens with float(lm * final) added; ties by (HCLG state, rank)
  if (w == 0) {
    const int fT0 = ftok[T], fT1 = min(ftok[T + 1], ntok);
    auto item = [&](int j) -> NbItem {
      NbItem it{-1, 0.f, 0, 0, 0, 0, 0};
      const int i = fT0 + j;
      if (!(tf[i] < INFINITY)) return it;
      it.src = i; it.add = (float)(p.lm * (double)tf[i]); it.fs = (uint32_t)tst[i]; it.bp = i;
      return it;
    };
    nb_merge(p, ec, eh, en, max(0, fT1 - fT0), item, acc, out, p.f_cost + (int64_t)n * K, p.f_bp + (int64_t)n * K,
             p.distinct ? p.f_hash + (int64_t)n * K : nullptr, p.f_n + n);
  }
}

// One lane per path: walk the back-pointers from the final entry to the start token.  path_nlab < 0: the path's labels did
// not fit label_cap (-1) or the walk did not end at frame 0 (-2).  Reference mode then drops a path whose label sequence
// equals an earlier path's; hyp_path[m] = path of hypothesis m, num_hyp = M.
__global__ void __launch_bounds__(64) nb_backtrace(NbParams p) {
  const int n = blockIdx.x, k = threadIdx.x, K = p.K;
  if (!p.ok[n]) { if (k == 0) p.num_hyp[n] = 0; return; }
  const LatUtt U = p.L.utt[n];
  const int T = U.T;
  const int64_t toff = p.tok_off[n], loff = p.link_off[n];
  const int2* eb = p.e_bp + toff * K;
  const int4* lrec = p.L.link_rec + U.link_base;
  const int32_t* lab = p.lab + loff;
  const int nf = p.f_n[n];
  const int64_t pk = (int64_t)n * K + k;
  int32_t* L = p.path_labels + pk * p.label_cap;
  int nlab = 0;
  uint64_t h = kNbHash0;
  if (k < nf) {
    const int2 f = p.f_bp[pk];
    int32_t* tids = p.path_tids + pk * p.Tmax;
    int tok = f.x, rank = f.y, fr = T;
    for (int steps = 0; steps <= U.n_link + 1; ++steps) {
      if ((unsigned)tok >= (unsigned)U.n_tok || rank < 0 || rank >= K) { fr = -1; break; }
      const int2 b = eb[(int64_t)tok * K + rank];
      if (b.x < 0) break;
      if (b.x >= U.n_link) { fr = -1; break; }
      const int4 r = lrec[b.x];
      if (r.z > 0) { --fr; if (fr >= 0 && fr < T) tids[fr] = r.z; }
      const int32_t lb = lab[b.x];
      if (lb != 0) { if (nlab < p.label_cap) L[nlab] = lb; ++nlab; h = nb_hash_step(h, lb); }
      tok = r.x; rank = b.y;
    }
    for (int i = 0, j = min(nlab, p.label_cap) - 1; i < j; ++i, --j) { const int32_t x = L[i]; L[i] = L[j]; L[j] = x; }
    if (nlab > p.label_cap) nlab = -1;
    if (fr != 0) nlab = -2;
    p.path_nlab[pk] = nlab; p.path_cost[pk] = p.f_cost[pk]; p.path_hash[pk] = h;
  }
  __syncthreads();
  bool keep = k < nf;
  if (keep && !p.distinct && nlab >= 0) {
    for (int k2 = 0; k2 < k && keep; ++k2) {
      const int64_t p2 = (int64_t)n * K + k2;
      if (p.path_hash[p2] != h || p.path_nlab[p2] != nlab) continue;
      const int32_t* L2 = p.path_labels + p2 * p.label_cap;
      bool same = true;
      for (int i = 0; i < nlab && same; ++i) same = L2[i] == L[i];
      if (same) keep = false;
    }
  }
  const uint64_t mask = __ballot(keep);
  const int m = __popcll(mask & ((1ull << k) - 1ull));
  if (keep) p.hyp_path[(int64_t)n * K + m] = k;
  if (k == 0) p.num_hyp[n] = __popcll(mask);
}

struct MweParams {
  int32_t N, Tmax, K, P, label_cap, equal_weight;
  const int32_t* ok; const int32_t* num_hyp; const int32_t* hyp_path; const float* path_cost; const int32_t* path_nlab;
  const int32_t* path_labels; const int32_t* path_tids;
  const int32_t* sup; int64_t sup_stride; const int32_t* sup_len;
  const int32_t* tid2pdf; int32_t num_tids;
  int32_t* ek; double* gk;
  float* grad; int64_t grad_seq_stride, grad_frame_stride;
  double* loss;
  const LatUtt* utt;
};

// Levenshtein distance (unit costs) of hypothesis m and the supervision (lattice_edit.h).
__global__ void __launch_bounds__(64) mwe_edit(MweParams p) {
  const int n = blockIdx.y, m = blockIdx.x, lane = threadIdx.x;
  if (!p.ok[n] || m >= p.num_hyp[n]) return;
  const int64_t pk = (int64_t)n * p.K + p.hyp_path[(int64_t)n * p.K + m];
  const int a = p.path_nlab[pk], b = p.sup_len[n];
  if (a < 0 || b < 0 || b > 64 * kEdChunks - 1) { if (lane == 0) p.ek[(int64_t)n * p.K + m] = -1; return; }
  const int32_t* x = p.path_labels + pk * p.label_cap;
  const int32_t* y = p.sup + (int64_t)n * p.sup_stride;
  const int e = edit_wave(x, a, y, b, lane);
  if (lane == 0) p.ek[(int64_t)n * p.K + m] = e;
}

__global__ void mwe_loss(MweParams p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.N) return;
  const int M = p.ok[n] ? p.num_hyp[n] : 0;
  const int64_t o = (int64_t)n * p.K;
  bool bad = M <= 0;
  for (int m = 0; m < M; ++m) bad |= p.ek[o + m] < 0;
  if (bad) {
    p.loss[n] = NAN;
    for (int m = 0; m < p.K; ++m) p.gk[o + m] = 0.0;
    return;
  }
  double wmin = INFINITY;
  for (int m = 0; m < M; ++m) wmin = fmin(wmin, (double)p.path_cost[o + p.hyp_path[o + m]]);
  double z = 0.0;
  for (int m = 0; m < M; ++m) z += p.equal_weight ? 1.0 : exp(-((double)p.path_cost[o + p.hyp_path[o + m]] - wmin));
  double loss = 0.0;
  for (int m = 0; m < M; ++m) {
    const double pm = p.equal_weight ? 1.0 / M : exp(-((double)p.path_cost[o + p.hyp_path[o + m]] - wmin)) / z;
    p.gk[o + m] = pm;
    loss += (double)p.ek[o + m] * pm;
  }
  for (int m = 0; m < M; ++m) p.gk[o + m] = ((double)p.ek[o + m] - loss) * p.gk[o + m];
  p.loss[n] = loss;
}

// grad[t, pdf] = sum over the hypotheses (in order) whose transition-id at frame t maps to pdf of g_k; one thread per frame.
__global__ void mwe_grad(MweParams p) {
  const int n = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (!p.ok[n] || t >= p.utt[n].T) return;
  const int M = p.num_hyp[n];
  const int64_t o = (int64_t)n * p.K;
  if (M <= 0) return;
  bool bad = false;
  for (int m = 0; m < M; ++m) bad |= p.ek[o + m] < 0;
  if (bad) return;
  float* row = p.grad + (int64_t)n * p.grad_seq_stride + (int64_t)t * p.grad_frame_stride;
  auto pdf_of = [&](int m) {
    const int tid = p.path_tids[(o + p.hyp_path[o + m]) * p.Tmax + t];
    return (tid >= 1 && tid <= p.num_tids) ? p.tid2pdf[tid] : -1;
  };
  for (int m = 0; m < M; ++m) {
    const int pdf = pdf_of(m);
    if (pdf < 0 || pdf >= p.P) continue;
    bool first = true;
    for (int m2 = 0; m2 < m && first; ++m2) first = pdf_of(m2) != pdf;
    if (!first) continue;
    double s = 0.0;
    for (int m2 = m; m2 < M; ++m2) if (pdf_of(m2) == pdf) s += p.gk[o + m2];
    row[pdf] = (float)s;
  }
}

// Scratch layout (base null: size only).
struct NbScratch {
  int64_t* tok_off; int64_t* link_off; int32_t* ok;
  float* e_cost; int2* e_bp; uint64_t* e_hash; int32_t* e_n; int32_t* lab; int32_t* gC; int32_t* gI; int32_t* gAd;
  int32_t* gAn;
  float* f_cost; int2* f_bp; uint64_t* f_hash; int32_t* f_n;
  int32_t* num_hyp; int32_t* hyp_path; float* path_cost; int32_t* path_nlab; int32_t* path_labels; int32_t* path_tids;
  uint64_t* path_hash; int32_t* ek; double* gk;
};
static size_t nb_carve(const pk2_lattice_batch* b, int K, int64_t ttot, int64_t ltot, int distinct, int label_cap,
                       void* base, NbScratch* s) {
  Carver c(base);
  const size_t N = b->N, NK = N * (size_t)K;
  s->tok_off = c.take<int64_t>(N); s->link_off = c.take<int64_t>(N); s->ok = c.take<int32_t>(N);
  s->e_cost = c.take<float>((size_t)ttot * K); s->e_bp = c.take<int2>((size_t)ttot * K);
  s->e_hash = distinct ? c.take<uint64_t>((size_t)ttot * K) : nullptr;
  s->e_n = c.take<int32_t>((size_t)ttot);
  s->lab = c.take<int32_t>((size_t)ltot);
  s->gC = c.take<int32_t>((size_t)ttot + N * (size_t)(b->Tmax + 2));
  s->gI = c.take<int32_t>((size_t)ltot); s->gAd = c.take<int32_t>((size_t)ltot); s->gAn = c.take<int32_t>((size_t)ltot);
  s->f_cost = c.take<float>(NK); s->f_bp = c.take<int2>(NK); s->f_hash = c.take<uint64_t>(NK); s->f_n = c.take<int32_t>(N);
  s->num_hyp = c.take<int32_t>(N); s->hyp_path = c.take<int32_t>(NK); s->path_cost = c.take<float>(NK);
  s->path_nlab = c.take<int32_t>(NK); s->path_labels = c.take<int32_t>(NK * (size_t)label_cap);
  s->path_tids = c.take<int32_t>(NK * (size_t)b->Tmax); s->path_hash = c.take<uint64_t>(NK);
  s->ek = c.take<int32_t>(NK); s->gk = c.take<double>(NK);
  return c.bytes();
}

// Output labels of the arcs and, per state, its arcs in (destination, transition-id, arc) order: uploaded by the first
// N-best call (decoding never reads them).
static int olabels_upload(pk2_decode_graph* g) {
  if (g->dev_ol_uploaded) return PK2_OK;
  for (int k = 0; k < 2; ++k) {
    const bool em = k == 0;
    const std::vector<int32_t>& off = em ? g->e_off : g->n_off;
    const std::vector<int32_t>& dst = em ? g->e_dst : g->n_dst;
    std::vector<int32_t> perm(dst.size());
    for (int32_t s = 0; s < g->S; ++s) {
      for (int32_t a = off[s]; a < off[s + 1]; ++a) perm[a] = a;
      std::sort(perm.begin() + off[s], perm.begin() + off[s + 1], [&](int32_t x, int32_t y) {
        if (dst[x] != dst[y]) return dst[x] < dst[y];
        if (em && g->e_tid[x] != g->e_tid[y]) return g->e_tid[x] < g->e_tid[y];
        return x < y;
      });
    }
    for (int j = 0; j < 2; ++j) {
      const std::vector<int32_t>& v = j == 0 ? (em ? g->e_ol : g->n_ol) : perm;
      void* d = nullptr;
      PK2_HIP(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(int32_t)));
      g->allocs.push_back(d);
      if (!v.empty()) PK2_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      const int32_t* dp = static_cast<const int32_t*>(d);
      if (j == 0) (em ? g->dev_e_ol : g->dev_n_ol) = dp; else (em ? g->dev_e_perm : g->dev_n_perm) = dp;
    }
  }
  g->dev_ol_uploaded = true;
  return PK2_OK;
}

static int nb_run(const pk2_lattice_batch* b, void* workspace, void* scratch, int64_t ttot, int64_t ltot, int32_t K,
                  int32_t distinct, int32_t label_mode, const int32_t* tid2label, int32_t num_tids, double lm, double am,
                  int32_t label_cap, NbScratch& s, NbParams& p, hipStream_t stream) {
  PK2_REQUIRE(b && workspace && scratch, "lattice nbest: null pointer");
  PK2_REQUIRE(b->decoded, "lattice nbest: pk2_lattice_decode has not run on this batch");
  PK2_REQUIRE(K >= 1 && K <= kNbMaxPaths, "lattice nbest: num_paths must be in 1..%d, got %d", kNbMaxPaths, K);
  PK2_REQUIRE(label_mode == 0 || label_mode == 1, "lattice nbest: label mode must be 0 (words) or 1 (phones)");
  PK2_REQUIRE(label_cap >= 1 && ttot >= 0 && ltot >= 0, "lattice nbest: bad sizes");
  PK2_REQUIRE(label_mode == 0 || (tid2label && num_tids >= 0), "lattice nbest: phone labels need the tid -> phone table");
  auto* g = const_cast<pk2_decode_graph*>(b->graph);
  PK2_REQUIRE(label_mode == 1 || g->has_olabels, "lattice nbest: the decoding graph carries no output labels (words)");
  PK2_REQUIRE(g->uploaded, "lattice nbest: decoding graph is not on the device");
  if (label_mode == 0) { const int rc = olabels_upload(g); if (rc) return rc; }
  nb_carve(b, K, ttot, ltot, distinct, label_cap, scratch, &s);
  p = NbParams{};
  lattice_carve(b, workspace, &p.L);
  p.N = b->N; p.Tmax = b->Tmax; p.K = K; p.distinct = distinct ? 1 : 0; p.label_cap = label_cap;
  // LDS left by the merge lists: a frame of up to `cap` tokens and `lcap` kept links is grouped there
  const size_t lists = (size_t)kNbWaves * 2 * K * sizeof(NbE);
  const int room = (int)((kNbLds - lists - 256) / sizeof(int32_t));
  const int lcap = std::min(4096, room / 4);
  const char* cap_env = getenv("PK2_NB_CAP");            // (test hook: 0 groups every frame's links in global memory)
  p.lcap = cap_env ? std::max(0, std::min(lcap, atoi(cap_env))) : lcap;
  p.cap = cap_env ? std::max(0, std::min(room - 3 * lcap, atoi(cap_env))) : room - 3 * lcap;
  p.lm = lm; p.am = am; p.tok_total = ttot; p.link_total = ltot;
  p.label_mode = label_mode; p.tid2label = tid2label; p.num_tids = num_tids;
  p.G = g->dev; p.e_ol = g->dev_e_ol; p.n_ol = g->dev_n_ol; p.e_perm = g->dev_e_perm; p.n_perm = g->dev_n_perm;
  p.tok_off = s.tok_off; p.link_off = s.link_off; p.ok = s.ok;
  p.e_cost = s.e_cost; p.e_bp = s.e_bp; p.e_hash = s.e_hash; p.e_n = s.e_n; p.lab = s.lab; p.gC = s.gC; p.gI = s.gI;
  p.gAd = s.gAd; p.gAn = s.gAn;
  p.f_cost = s.f_cost; p.f_bp = s.f_bp; p.f_hash = s.f_hash; p.f_n = s.f_n;
  p.num_hyp = s.num_hyp; p.hyp_path = s.hyp_path; p.path_cost = s.path_cost; p.path_nlab = s.path_nlab;
  p.path_labels = s.path_labels; p.path_tids = s.path_tids; p.path_hash = s.path_hash;
  const size_t smem = lists + (size_t)(p.cap + 3 * p.lcap) * sizeof(int32_t);
  PK2_DYN_LDS_ONCE(nb_kbest, kNbLds);
  hipLaunchKernelGGL(nb_prep, dim3(1), dim3(64), 0, stream, p);
  hipLaunchKernelGGL(nb_labels, dim3(2 * (b->Tmax + 1), b->N), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(nb_kbest, dim3(b->N), dim3(kNbThreads), smem, stream, p);
  hipLaunchKernelGGL(nb_backtrace, dim3(b->N), dim3(64), 0, stream, p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_lattice_nbest_bytes(const pk2_lattice_batch* b, int32_t num_paths, int64_t total_tokens,
                                          int64_t total_links, int32_t distinct, int32_t label_cap) {
  if (!b || num_paths < 1 || num_paths > kNbMaxPaths || label_cap < 1) return 0;
  NbScratch s;
  return nb_carve(b, num_paths, total_tokens, total_links, distinct, label_cap, nullptr, &s);
}

extern "C" int pk2_lattice_nbest(const pk2_lattice_batch* b, void* workspace, void* scratch, int64_t total_tokens,
                                 int64_t total_links, int32_t num_paths, int32_t distinct, int32_t label_mode,
                                 const int32_t* tid2label, int32_t num_tids, double lm_scale, double acoustic_scale,
                                 int32_t label_cap, int32_t* num_hyp, int32_t* hyp_path, float* path_cost,
                                 int32_t* path_nlab, int32_t* path_labels, int32_t* path_tids, void* stream_) {
  PK2_REQUIRE(num_hyp && hyp_path && path_cost && path_nlab && path_labels && path_tids, "lattice nbest: null output");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  NbScratch s; NbParams p;
  int rc = nb_run(b, workspace, scratch, total_tokens, total_links, num_paths, distinct, label_mode, tid2label, num_tids,
                  lm_scale, acoustic_scale, label_cap, s, p, stream);
  if (rc) return rc;
  const size_t NK = (size_t)b->N * num_paths;
  PK2_HIP(hipMemcpyAsync(num_hyp, s.num_hyp, sizeof(int32_t) * b->N, hipMemcpyDeviceToDevice, stream));
  PK2_HIP(hipMemcpyAsync(hyp_path, s.hyp_path, sizeof(int32_t) * NK, hipMemcpyDeviceToDevice, stream));
  PK2_HIP(hipMemcpyAsync(path_cost, s.path_cost, sizeof(float) * NK, hipMemcpyDeviceToDevice, stream));
  PK2_HIP(hipMemcpyAsync(path_nlab, s.path_nlab, sizeof(int32_t) * NK, hipMemcpyDeviceToDevice, stream));
  PK2_HIP(hipMemcpyAsync(path_labels, s.path_labels, sizeof(int32_t) * NK * label_cap, hipMemcpyDeviceToDevice, stream));
  PK2_HIP(hipMemcpyAsync(path_tids, s.path_tids, sizeof(int32_t) * NK * b->Tmax, hipMemcpyDeviceToDevice, stream));
  return PK2_OK;
}

extern "C" int pk2_lattice_mwe(const pk2_lattice_batch* b, void* workspace, void* scratch, int64_t total_tokens,
                               int64_t total_links, int32_t num_paths, int32_t distinct, int32_t label_mode,
                               const int32_t* tid2label, int32_t num_tids, double lm_scale, double acoustic_scale,
                               int32_t label_cap, int32_t equal_weight, const int32_t* sup, int64_t sup_stride,
                               const int32_t* sup_len, const int32_t* tid2pdf, int32_t num_pdfs, float* grad,
                               int64_t grad_seq_stride, int64_t grad_frame_stride, double* loss, void* stream_) {
  PK2_REQUIRE(sup && sup_len && tid2pdf && grad && loss, "lattice mwe: null pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  NbScratch s; NbParams p;
  int rc = nb_run(b, workspace, scratch, total_tokens, total_links, num_paths, distinct, label_mode, tid2label, num_tids,
                  lm_scale, acoustic_scale, label_cap, s, p, stream);
  if (rc) return rc;
  MweParams m{};
  m.N = b->N; m.Tmax = b->Tmax; m.K = num_paths; m.P = num_pdfs; m.label_cap = label_cap; m.equal_weight = equal_weight ? 1 : 0;
  m.ok = s.ok; m.num_hyp = s.num_hyp; m.hyp_path = s.hyp_path; m.path_cost = s.path_cost; m.path_nlab = s.path_nlab;
  m.path_labels = s.path_labels; m.path_tids = s.path_tids;
  m.sup = sup; m.sup_stride = sup_stride; m.sup_len = sup_len; m.tid2pdf = tid2pdf; m.num_tids = num_tids;
  m.ek = s.ek; m.gk = s.gk; m.grad = grad; m.grad_seq_stride = grad_seq_stride; m.grad_frame_stride = grad_frame_stride;
  m.loss = loss; m.utt = p.L.utt;
  hipLaunchKernelGGL(mwe_edit, dim3(num_paths, b->N), dim3(64), 0, stream, m);
  hipLaunchKernelGGL(mwe_loss, dim3((b->N + 63) / 64), dim3(64), 0, stream, m);
  hipLaunchKernelGGL(mwe_grad, dim3((b->Tmax + 255) / 256, b->N), dim3(256), 0, stream, m);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
