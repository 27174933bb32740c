// N-gram LM rescoring of packed word lattices (include/pk2hip.h: pk2_ngram_*, pk2_wordlat_lmrescore):
// on-the-fly composition of a lattice with a deterministic backoff LM (Kaldi's lattice-lmrescore-const-arpa, restated).
//
//   lr_kernel   one workgroup of 1024 threads per lattice, gather form, the input levels upward.  Per level:
//               (1) one thread per incoming arc: |pairs(source)|, a workgroup scan over the level's arcs gives every
//                   candidate (arc a, pair index j) its slot = the output arc ranges of the level's states;
//               (2) every candidate does one LM lookup (binary searches along the backoff chain) and gets the key
//                   (h' << 32) | candidate index; the candidates of a state are sorted by key: one wave per state in
//                   registers up to 64 candidates, the whole workgroup in LDS up to PK2_LMRESCORE_SORT_LDS, in the
//                   workspace above; the end state is not sorted (every h' is 0), its candidates go over all threads;
//               (3) run boundaries of h' are the new states: a second workgroup scan numbers them.
//
// Integer arithmetic, one float64 sum per lookup in a fixed order, one float32 rounding per arc: every output bit is a
// function of the inputs.  No atomics on floats, no waiting between workgroups.  A lattice whose room (expand S states,
// expand A arcs) is short stops with status 2 before anything is written beyond its share.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "wordlat.h"

#pragma clang fp contract(off)

namespace pk2 {
namespace {

constexpr int kLrThreads = 1024;
constexpr int kLrWaves = kLrThreads / 64;
static_assert((PK2_LMRESCORE_SORT_LDS & (PK2_LMRESCORE_SORT_LDS - 1)) == 0 && PK2_LMRESCORE_SORT_LDS >= 128, "bitonic sort: a power of two");
constexpr int64_t kLrMaxRoom = (int64_t)1 << 29;     // states / arcs of one composed lattice

struct NgramDev {
  int32_t N = 0, order = 0, start = 0, eos = 0;
  void* blob = nullptr;
  const int32_t *d_word, *d_child, *d_bo, *d_next;
  const float *d_cost, *d_backoff;
};

struct LrParams {
  const int64_t *state_off, *arc_off, *level_off_off, *word_off_off;
  const int32_t *src, *dst, *word, *in_off, *level_off, *word_ids, *lm_word;
  const float *graph, *acoustic;
  const int32_t *n_word, *n_child, *n_bo, *n_next;
  const float *n_cost, *n_backoff;
  int32_t lm_start, lm_eos, first;
  double scale, expand;
  unsigned long long* work;
  int32_t *o_nstates, *o_narcs, *status;
  pk2_lm_state* states;
  pk2_lm_arc* arcs;
};

struct LrTmp { int32_t h; float g; int32_t hn; };    // per output arc slot: h' of the sorted arc | new graph cost, h' of the candidate

__host__ __device__ inline int64_t lr_room(double expand, int64_t n) { return (int64_t)(expand * (double)n); }
// 8-byte words of workspace of one lattice: [keys 2 capA | pair_off S + 1, cand_pre A + 1 (int32), tmp capA x 12 bytes]
__host__ __device__ inline int64_t lr_work_words(int64_t S, int64_t A, int64_t capA) {
  return 2 * capA + (S + 1 + A + 1 + 3 * capA + 1) / 2;
}

__device__ __forceinline__ unsigned long long lr_shfl_xor64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ long long lr_shfl_up64(long long v, int o) {
  const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)((unsigned long long)v >> 32), o, 64);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// cost and next state of word w from LM state h (arc(h, w)); false if w has no unigram
__device__ __forceinline__ bool lr_lm_arc(const LrParams& p, int h, int w, double& cost, int& next) {
  double acc = 0.0;
  int node = h;
#pragma nounroll
  for (int it = 0; it <= PK2_NGRAM_MAX_ORDER; ++it) {
    const int end = p.n_child[node + 1];
    int lo = p.n_child[node], hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.n_word[mid] < w) lo = mid + 1; else hi = mid;
    }
    if (lo < end && p.n_word[lo] == w) { cost = acc + (double)p.n_cost[lo]; next = p.n_next[lo]; return true; }
    if (node == 0) break;
    acc += (double)p.n_backoff[node];
    node = p.n_bo[node];
  }
  cost = 0.0; next = 0;
  return false;
}

// Inclusive scan in place of v[0..n) (values >= 0) on top of `carry`, by the whole workgroup; values beyond int32 are
// stored as INT32_MAX (the caller then stops on the returned total).  Ends with a barrier.
__device__ __forceinline__ long long lr_block_scan(int32_t* v, int stride, int n, long long carry, long long* sh_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma nounroll
  for (int base = 0; base < n; base += kLrThreads) {
    const int i = base + tid;
    long long x = i < n ? (long long)v[(int64_t)i * stride] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long y = lr_shfl_up64(x, o); if (lane >= o) x += y; }
    if (lane == 63) sh_wave[wave] = x;
    __syncthreads();
    if (tid < kLrWaves) {               // the wave totals' own prefix, by the first lanes of wave 0
      long long y = sh_wave[tid];
#pragma unroll
      for (int o = 1; o < kLrWaves; o <<= 1) { const long long z = lr_shfl_up64(y, o); if (tid >= o) y += z; }
      sh_wave[kLrWaves + tid] = y;
    }
    __syncthreads();
    const long long before = wave > 0 ? sh_wave[kLrWaves + wave - 1] : 0, tot = sh_wave[2 * kLrWaves - 1];
    const long long r = carry + before + x;
    if (i < n) v[(int64_t)i * stride] = r > 0x7fffffffLL ? 0x7fffffff : (int32_t)r;
    carry += tot;
    __syncthreads();
  }
  return carry;
}

struct LrLat {
  int S, A, depth;
  const int32_t *src, *dst, *word, *in_off, *level_off, *word_ids, *lm_word;
  const float *graph, *acoustic;
  unsigned long long* keys;
  LrTmp* tmp;
  int32_t *pair_off, *cand_pre;
  pk2_lm_state* states;
  pk2_lm_arc* arcs;
};

// the incoming arc that holds candidate slot x: the last a in [lo, hi) with cand_pre[a] <= x
__device__ __forceinline__ int lr_find_arc(const LrLat& L, int lo, int hi, int x) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.cand_pre[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// output arc o of state n <- candidate slot x
__device__ __forceinline__ void lr_emit(const LrLat& L, int n, int o, int x) {
  const int a = lr_find_arc(L, L.in_off[n], L.in_off[n + 1], x);
  pk2_lm_arc r;
  r.src = L.pair_off[L.src[a]] + (x - L.cand_pre[a]); r.dst = 0; r.word = L.word_ids[L.word[a]]; r.orig = a;
  r.graph = L.tmp[x].g; r.acoustic = L.acoustic[a];
  L.arcs[o] = r;
  L.tmp[o].h = L.tmp[x].hn;
}

// bitonic sort of keys[0..n2) (n2 a power of two) by the whole workgroup; keys in LDS or in the workspace
template <class K>
__device__ __forceinline__ void lr_block_sort(K keys, int n2) {
  for (int k = 2; k <= n2 && k > 0; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma nounroll
      for (int i = threadIdx.x; i < n2; i += kLrThreads) {
        const int q = i ^ j;
        if (q > i) {
          const unsigned long long x = keys[i], y = keys[q];
          if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[q] = x; }
        }
      }
      __threadfence_block();
      __syncthreads();
    }
  }
}

// one state of more than 64 candidates, by the whole workgroup
template <class K>
__device__ __forceinline__ void lr_big_state(const LrLat& L, int n, int base, int cnt, int n2, K keys) {
#pragma nounroll
  for (int i = threadIdx.x; i < n2; i += kLrThreads)
    keys[i] = i < cnt ? ((unsigned long long)(unsigned)L.tmp[base + i].hn << 32) | (unsigned)i : ~0ull;
  __threadfence_block();
  __syncthreads();
  lr_block_sort(keys, n2);
#pragma nounroll
  for (int i = threadIdx.x; i < cnt; i += kLrThreads) lr_emit(L, n, base + i, base + (int)(unsigned)keys[i]);
  __syncthreads();
}

__global__ void __launch_bounds__(kLrThreads) lr_kernel(LrParams p) {
  __shared__ unsigned long long sh_keys[PK2_LMRESCORE_SORT_LDS];
  __shared__ long long sh_wave[2 * kLrWaves];
  __shared__ int32_t sh_list[kLrThreads];
  __shared__ int32_t sh_n, sh_fail;
  const int li = blockIdx.x, l = p.first + li, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // this lattice's share of the outputs and of the workspace
  int64_t sbase = 0, abase = 0, wbase = 0;
  for (int k = p.first; k < l; ++k) {
    const int64_t S = p.state_off[k + 1] - p.state_off[k], A = p.arc_off[k + 1] - p.arc_off[k];
    sbase += lr_room(p.expand, S); abase += lr_room(p.expand, A);
    wbase += lr_work_words(S, A, lr_room(p.expand, A));
  }
  LrLat L;
  const int64_t so = p.state_off[l], ao = p.arc_off[l], lo = p.level_off_off[l], wo = p.word_off_off[l];
  L.S = (int)(p.state_off[l + 1] - so); L.A = (int)(p.arc_off[l + 1] - ao);
  L.depth = (int)(p.level_off_off[l + 1] - lo) - 2;
  const int64_t capS = lr_room(p.expand, L.S), capA = lr_room(p.expand, L.A);
  L.src = p.src + ao; L.dst = p.dst + ao; L.word = p.word + ao; L.graph = p.graph + ao; L.acoustic = p.acoustic + ao;
  L.in_off = p.in_off + so + l; L.level_off = p.level_off + lo; L.word_ids = p.word_ids + wo - l; L.lm_word = p.lm_word + wo - l;
  L.keys = p.work + wbase;
  L.pair_off = reinterpret_cast<int32_t*>(L.keys + 2 * capA);
  L.cand_pre = L.pair_off + L.S + 1;
  L.tmp = reinterpret_cast<LrTmp*>(L.cand_pre + L.A + 1);
  L.states = p.states + sbase; L.arcs = p.arcs + abase;

  int status = (capS < 1 || capA < 1) ? 2 : 0;
  long long narcs = 0, nstates = 1;
  if (tid == 0) {
    sh_fail = 0;
    L.pair_off[0] = 0; L.pair_off[1] = 1; L.cand_pre[0] = 0;
    if (status == 0) { L.states[0].s = 0; L.states[0].h = p.lm_start; }
  }
  __threadfence_block();
  __syncthreads();
  int fail = 0;
  for (int lev = 1; lev <= L.depth && status == 0; ++lev) {
    const int s0 = L.level_off[lev], s1 = L.level_off[lev + 1], a0 = L.in_off[s0], a1 = L.in_off[s1];
    // (1) candidates per incoming arc, and their slots
#pragma nounroll
    for (int a = a0 + tid; a < a1; a += kLrThreads) { const int u = L.src[a]; L.cand_pre[a + 1] = L.pair_off[u + 1] - L.pair_off[u]; }
    __threadfence_block();
    __syncthreads();
    const long long total = lr_block_scan(L.cand_pre + a0 + 1, 1, a1 - a0, narcs, sh_wave);
    if (total > capA) { status = 2; break; }
    const int x0 = (int)narcs, x1 = (int)total;
    const bool last = lev == L.depth;
    // (2a) one LM lookup per candidate, the level's candidates over all threads
#pragma nounroll
    for (int x = x0 + tid; x < x1; x += kLrThreads) {
      const int a = lr_find_arc(L, a0, a1, x);
      const int h = L.states[L.pair_off[L.src[a]] + (x - L.cand_pre[a])].h, w = L.word[a];
      double cost = 0.0;
      int hn = h;
      if (last) {
        if (!lr_lm_arc(p, h, p.lm_eos, cost, hn)) fail = 1;
        hn = 0;
      } else if (w != 0) {
        if (!lr_lm_arc(p, h, L.lm_word[w], cost, hn)) fail = 1;
      }
      L.tmp[x].g = (float)((double)L.graph[a] + p.scale * cost);
      L.tmp[x].hn = hn;
    }
    __threadfence_block();
    __syncthreads();
    // (2b) the candidates of a state sorted by (h', slot) are its arcs
    if (last) {                         // the end state: every h' is 0
#pragma nounroll
      for (int x = x0 + tid; x < x1; x += kLrThreads) lr_emit(L, L.S - 1, x, x);
    } else {
#pragma nounroll
      for (int n = s0 + wave; n < s1; n += kLrWaves) {      // a wave per state of at most 64 candidates
        const int base = L.cand_pre[L.in_off[n]], cnt = L.cand_pre[L.in_off[n + 1]] - base;
        if (cnt > 64) continue;
        unsigned long long key = ~0ull;
        if (lane < cnt) key = ((unsigned long long)(unsigned)L.tmp[base + lane].hn << 32) | (unsigned)lane;
#pragma nounroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma nounroll
          for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long other = lr_shfl_xor64(key, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            key = (other < key) == keep_min ? other : key;
          }
        }
        if (lane < cnt) lr_emit(L, n, base + lane, base + (int)(key & 63u));
      }
      for (int c0 = s0; c0 < s1; c0 += kLrThreads) {          // the large states of the level, one after the other
        __syncthreads();
        if (tid == 0) sh_n = 0;
        __syncthreads();
        const int n_ = c0 + tid;
        if (n_ < s1 && L.cand_pre[L.in_off[n_ + 1]] - L.cand_pre[L.in_off[n_]] > 64) sh_list[atomicAdd(&sh_n, 1)] = n_;
        __syncthreads();
        const int nbig = sh_n;
        for (int b = 0; b < nbig; ++b) {
          const int n = sh_list[b];
          const int base = L.cand_pre[L.in_off[n]], cnt = L.cand_pre[L.in_off[n + 1]] - base;
          int n2 = 128;
          while (n2 < cnt) n2 <<= 1;
          if (cnt <= PK2_LMRESCORE_SORT_LDS) lr_big_state(L, n, base, cnt, n2, sh_keys);
          else lr_big_state(L, n, base, cnt, n2, L.keys);
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    // (3) a new state wherever h' changes inside a state's arcs; dst holds the flag, then the state's number
#pragma nounroll
    for (int x = x0 + tid; x < x1; x += kLrThreads) {
      const int n = L.dst[L.arcs[x].orig];
      L.arcs[x].dst = (x == L.cand_pre[L.in_off[n]] || L.tmp[x - 1].h != L.tmp[x].h) ? 1 : 0;
    }
    __threadfence_block();
    __syncthreads();
    const long long totalS = lr_block_scan(&L.arcs[x0].dst, (int)(sizeof(pk2_lm_arc) / 4), x1 - x0, nstates, sh_wave);
    if (totalS > capS) { status = 2; break; }
#pragma nounroll
    for (int x = x0 + tid; x < x1; x += kLrThreads) {
      const int n = L.dst[L.arcs[x].orig], pr = L.arcs[x].dst - 1;
      L.arcs[x].dst = pr;
      if (x == L.cand_pre[L.in_off[n]] || L.tmp[x - 1].h != L.tmp[x].h) { L.states[pr].s = n; L.states[pr].h = L.tmp[x].h; }
      if (x + 1 == L.cand_pre[L.in_off[n + 1]]) L.pair_off[n + 1] = pr + 1;
    }
    narcs = total; nstates = totalS;
    __threadfence_block();
    __syncthreads();
  }
  if (fail) sh_fail = 1;
  __syncthreads();
  if (tid == 0) {
    if (status == 0 && sh_fail) status = 3;
    p.status[li] = status;
    p.o_nstates[li] = status == 0 ? (int32_t)nstates : 0;
    p.o_narcs[li] = status == 0 ? (int32_t)narcs : 0;
  }
}

bool lr_range_ok(const WordLat* h, int first, int count) { return h && first >= 0 && count >= 1 && (int64_t)first + count <= h->N; }

// rooms of the range; false if a lattice's room is beyond what the kernel indexes
bool lr_sizes(const WordLat* h, int first, int count, double expand, int64_t& states, int64_t& arcs, int64_t& words) {
  states = arcs = words = 0;
  for (int l = first; l < first + count; ++l) {
    const int64_t S = h->state_off[l + 1] - h->state_off[l], A = h->arc_off[l + 1] - h->arc_off[l];
    if (expand * (double)S > (double)kLrMaxRoom || expand * (double)A > (double)kLrMaxRoom) return false;
    states += lr_room(expand, S); arcs += lr_room(expand, A);
    words += lr_work_words(S, A, lr_room(expand, A));
  }
  return true;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" int pk2_ngram_create(int32_t N, int32_t order, const int32_t* order_off, const int32_t* word, const float* cost,
                                const float* backoff, const int32_t* child_begin, const int32_t* bo_link,
                                const int32_t* next_state, int32_t start, int32_t eos, void* stream, void** out) {
  PK2_REQUIRE(out, "ngram_create: null output");
  *out = nullptr;
  PK2_REQUIRE(order_off && word && cost && backoff && child_begin && bo_link && next_state, "ngram_create: null pointer");
  PK2_REQUIRE(order >= 1 && order <= PK2_NGRAM_MAX_ORDER, "ngram_create: order %d (1..%d)", order, PK2_NGRAM_MAX_ORDER);
  PK2_REQUIRE(N >= 2, "ngram_create: %d nodes", N);
  // every index the kernel follows is checked here, once
  const char* bad = nullptr;
  if (order_off[0] != 0 || order_off[1] != 1 || order_off[order + 1] != N) bad = "order ranges";
  for (int k = 0; k <= order && !bad; ++k) if (order_off[k + 1] < order_off[k]) bad = "order ranges";
  std::vector<int32_t> lev(bad ? 0 : N);
  if (!bad) for (int k = 0; k <= order; ++k) for (int32_t i = order_off[k]; i < order_off[k + 1]; ++i) lev[i] = k;
  if (!bad && (child_begin[0] != 1 || child_begin[N] != N)) bad = "child ranges";
  for (int32_t i = 0; i < N && !bad; ++i) {
    const int32_t b = child_begin[i], e = child_begin[i + 1];
    if (e < b || b < 0 || e > N) { bad = "child ranges"; break; }
    if (e > b) {
      if (lev[i] >= order || b < order_off[lev[i] + 1] || e > order_off[lev[i] + 2]) { bad = "child range outside the next order"; break; }
      for (int32_t c = b; c < e; ++c) if (word[c] < 0 || (c > b && word[c] <= word[c - 1])) bad = "words of a child range not ascending";
    }
    if (!std::isfinite(cost[i]) || !std::isfinite(backoff[i])) bad = "non-finite weight";
  }
  auto has_children = [&](int32_t i) { return i >= 0 && i < N && child_begin[i + 1] > child_begin[i]; };
  for (int32_t i = 0; i < N && !bad; ++i) {
    if (bo_link[i] < 0 || bo_link[i] >= N || (i > 0 ? lev[bo_link[i]] >= lev[i] : bo_link[i] != 0)) bad = "backoff link";
    else if (next_state[i] != 0 && !has_children(next_state[i])) bad = "next state";
  }
  if (!bad && start != 0 && !has_children(start)) bad = "start state";
  if (!bad) {
    const int32_t* b = word + child_begin[0];
    const int32_t* e = word + child_begin[1];
    const int32_t* f = std::lower_bound(b, e, eos);
    if (f == e || *f != eos) bad = "no unigram for the end-of-sentence word";
  }
  if (bad) { set_error("ngram_create: malformed LM tables (%s)", bad); return PK2_ERR_INVALID; }
  NgramDev* h = new NgramDev;
  h->N = N; h->order = order; h->start = start; h->eos = eos;
  Carver sz(nullptr);
  auto carve = [&](Carver& c, NgramDev* o) {
    o->d_word = c.take<int32_t>(N); o->d_child = c.take<int32_t>(N + 1); o->d_bo = c.take<int32_t>(N);
    o->d_next = c.take<int32_t>(N); o->d_cost = c.take<float>(N); o->d_backoff = c.take<float>(N);
  };
  NgramDev dummy;
  carve(sz, &dummy);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMalloc(&h->blob, sz.bytes());
  if (e != hipSuccess) { delete h; set_error("ngram_create: hipMalloc(%zu) -> %s", sz.bytes(), hipGetErrorString(e)); return PK2_ERR_HIP; }
  Carver cv(h->blob);
  carve(cv, h);
  auto up = [&](const void* d, const void* s, size_t n) { if (e == hipSuccess && n) e = hipMemcpyAsync(const_cast<void*>(d), s, n, hipMemcpyHostToDevice, st); };
  up(h->d_word, word, 4 * (size_t)N); up(h->d_child, child_begin, 4 * ((size_t)N + 1)); up(h->d_bo, bo_link, 4 * (size_t)N);
  up(h->d_next, next_state, 4 * (size_t)N); up(h->d_cost, cost, 4 * (size_t)N); up(h->d_backoff, backoff, 4 * (size_t)N);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(h->blob);
    delete h;
    set_error("ngram_create: upload -> %s", hipGetErrorString(e));
    return PK2_ERR_HIP;
  }
  *out = h;
  return PK2_OK;
}

extern "C" int pk2_ngram_destroy(void* handle) {
  NgramDev* h = static_cast<NgramDev*>(handle);
  if (!h) return PK2_OK;
  if (h->blob) PK2_HIP(hipFree(h->blob));
  delete h;
  return PK2_OK;
}

extern "C" size_t pk2_wordlat_lmrescore_workspace_bytes(const void* handle, int32_t first, int32_t count, double expand) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  int64_t s, a, w;
  if (!lr_range_ok(h, first, count) || !std::isfinite(expand) || expand <= 0.0 || !lr_sizes(h, first, count, expand, s, a, w)) return 0;
  return (size_t)w * 8 + 8;
}

extern "C" int pk2_wordlat_lmrescore(const void* h_lat, int32_t first, int32_t count, const void* h_lm, const int32_t* lm_word,
                                     double scale, double expand, void* work, size_t work_bytes, int32_t* out_nstates,
                                     int32_t* out_narcs, pk2_lm_state* states, size_t state_room, pk2_lm_arc* arcs, size_t arc_room,
                                     int32_t* status, void* stream) {
  const WordLat* h = static_cast<const WordLat*>(h_lat);
  const NgramDev* lm = static_cast<const NgramDev*>(h_lm);
  PK2_REQUIRE(h && lm && lm_word && work && out_nstates && out_narcs && states && arcs && status, "wordlat_lmrescore: null pointer");
  PK2_REQUIRE(std::isfinite(scale), "wordlat_lmrescore: non-finite scale");
  PK2_REQUIRE(std::isfinite(expand) && expand > 0.0, "wordlat_lmrescore: expand must be finite and positive");
  PK2_REQUIRE(lr_range_ok(h, first, count), "wordlat_lmrescore: lattices %d..%d of %d", first, first + count, h->N);
  int64_t s, a, w;
  PK2_REQUIRE(lr_sizes(h, first, count, expand, s, a, w), "wordlat_lmrescore: expand %g gives a lattice more than 2^29 states or arcs", expand);
  PK2_REQUIRE(state_room >= (size_t)s && arc_room >= (size_t)a, "wordlat_lmrescore: room for %zu states and %zu arcs, need %lld and %lld",
              state_room, arc_room, (long long)s, (long long)a);
  PK2_REQUIRE(work_bytes >= (size_t)w * 8 + 8 && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_lmrescore: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, (size_t)w * 8 + 8);
  LrParams p;
  memset(&p, 0, sizeof(p));
  p.state_off = h->d_state_off; p.arc_off = h->d_arc_off; p.level_off_off = h->d_level_off_off; p.word_off_off = h->d_word_off_off;
  p.src = h->d_src; p.dst = h->d_dst; p.word = h->d_word; p.in_off = h->d_in_off; p.level_off = h->d_level_off;
  p.word_ids = h->d_word_ids; p.lm_word = lm_word; p.graph = h->d_graph; p.acoustic = h->d_acoustic;
  p.n_word = lm->d_word; p.n_child = lm->d_child; p.n_bo = lm->d_bo; p.n_next = lm->d_next; p.n_cost = lm->d_cost;
  p.n_backoff = lm->d_backoff; p.lm_start = lm->start; p.lm_eos = lm->eos; p.first = first; p.scale = scale; p.expand = expand;
  p.work = static_cast<unsigned long long*>(work);
  p.o_nstates = out_nstates; p.o_narcs = out_narcs; p.status = status; p.states = states; p.arcs = arcs;
  hipLaunchKernelGGL(lr_kernel, dim3(count), dim3(kLrThreads), 0, static_cast<hipStream_t>(stream), p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
