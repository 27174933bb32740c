// Word-boundary alignment of best-path word times (include/pk2hip.h: pk2_wordlat_set_strings, pk2_wordalign_model_*,
// pk2_wordlat_align_words): what the recipes' `lattice-1best | lattice-align-words | nbest-to-ctm` print, for
// every (lattice, setting) pair of a pk2_wordlat_best_path call.
//
//   wa_kernel   one workgroup of 4 wavefronts per pair.  Thread 0 walks the pair's back-pointers (at most depth steps); the
//               workgroup prefix-sums the arcs' string lengths and gathers, one wavefront per arc, the transition-state and
//               phone | flags of every frame into the pair's workspace.  SplitToPhones is a min-reduction (is the model
//               reordered?), one max-scan (has a transition to the final HMM state been seen since the last frame that is
//               not a same-transition-state self-loop?) and one sum-scan of the cut flags; the word-boundary grouping is a
//               segmented scan over the phones (token start, "a phone does not fit its place") and a sum-scan (token index,
//               rank among the word-bearing tokens).  Frames and phones are taken in chunks of the workgroup's size with the
//               scan carries in registers, so an utterance of any length runs; LDS holds two words per thread.
//
// Integers only, no atomics, nothing shared between workgroups: the same bits in a batch as in a single call.
#include <climits>
#include <vector>

#include "common.h"
#include "wordlat.h"

namespace pk2 {

struct WordAlignModel {
  int32_t num_tids = 0, num_phones = 0;
  void* blob = nullptr;
  const int2* d_tid = nullptr;       // per transition-id (entry 0 unused): x = transition-state, y = phone << 2 | flags & 3
  const uint8_t* d_cat = nullptr;    // per phone: 0 nonword, 1 begin, 2 end, 3 internal, 4 singleton, 255 no entry
};

namespace {

constexpr int kWaThreads = 256, kWaWaves = kWaThreads / 64;

struct WaParams {
  const int64_t *state_off, *arc_off, *level_off_off, *word_off_off, *tid_off, *align_pre;
  const int32_t *src, *word, *in_off, *word_ids, *tids, *fcap;
  const int2* tid_tab; const uint8_t* cat; int32_t num_phones;
  int32_t first, G;
  const int32_t *bp, *bp_status;
  int32_t* work;
  int32_t *path_times, *word_times, *tokens, *ntokens, *phones, *nphones, *status, *reason;
  int32_t word_stride, token_stride, phone_stride;
};

struct I2 { int32_t a, b; };
__device__ __forceinline__ int32_t wa_up(int32_t x, int d) { return __shfl_up(x, d, 64); }
__device__ __forceinline__ I2 wa_up(I2 x, int d) { return I2{__shfl_up(x.a, d, 64), __shfl_up(x.b, d, 64)}; }

// Inclusive scan over the workgroup's threads in thread order under an associative op, continued from `carry` (the
// scan of everything before this chunk; the op's identity at first); `carry` becomes the total, the same in every thread.
template <class T, class Op>
__device__ __forceinline__ T wa_scan(T x, Op op, T& carry, T* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const T y = wa_up(x, d); if (lane >= d) x = op(y, x); }
  if (lane == 63) sh[wave] = x;
  __syncthreads();
  T pre = carry;
#pragma unroll
  for (int w = 0; w < kWaWaves; ++w) { if (w == wave) x = op(pre, x); pre = op(pre, sh[w]); }
  __syncthreads();
  carry = pre;
  return x;
}

struct OpSum { __device__ int32_t operator()(int32_t a, int32_t b) const { return a + b; } };
struct OpMax { __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; } };
struct OpSum2 { __device__ I2 operator()(I2 a, I2 b) const { return I2{a.a + b.a, a.b + b.b}; } };
// segmented: a = index of the segment's first element (-1: the element continues a segment), b = OR over the segment
struct OpSeg { __device__ I2 operator()(I2 a, I2 b) const { return b.a >= 0 ? b : I2{a.a, a.b | b.b}; } };

__device__ __forceinline__ bool wa_starts_token(int c) { return c == 0 || c == 4 || c == 1; }
__device__ __forceinline__ bool wa_ends_token(int c) { return c == 0 || c == 4 || c == 2; }

__global__ void __launch_bounds__(kWaThreads) wa_kernel(WaParams p) {
  __shared__ int32_t sh_m[kWaThreads], sh_cut[kWaThreads], sh_w[kWaWaves], sh_na, sh_fail;
  __shared__ I2 sh_w2[kWaWaves];
  const int pair = blockIdx.x, li = pair / p.G, g = pair % p.G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = p.first + li;
  const int S = (int)(p.state_off[l + 1] - p.state_off[l]);
  const int depth = (int)(p.level_off_off[l + 1] - p.level_off_off[l]) - 2, fcap = p.fcap[l];
  const int32_t* src = p.src + p.arc_off[l];
  const int32_t* word = p.word + p.arc_off[l];
  const int32_t* in_off = p.in_off + p.state_off[l] + l;
  const int32_t* word_ids = p.word_ids + p.word_off_off[l] - l;
  const int64_t* tid_off = p.tid_off + p.arc_off[l];
  const int32_t* bp = p.bp + (int64_t)p.G * (p.state_off[l] - p.state_off[p.first]) + (int64_t)g * S;
  // the pair's workspace: [path depth | begin depth | label depth | transition-state fcap | phone,flags fcap | phone fcap | begin fcap]
  const int64_t per = 3 * (int64_t)depth + 4 * (int64_t)fcap;
  int32_t* ws = p.work + 2 * ((int64_t)p.G * (p.align_pre[l] - p.align_pre[p.first]) + (int64_t)g * ((per + 1) / 2));
  int32_t *path = ws, *pbeg = ws + depth, *plab = ws + 2 * (int64_t)depth, *fts = ws + 3 * (int64_t)depth, *fpf = fts + fcap;
  int32_t *php = fpf + fcap, *phb = php + fcap;
  int32_t* pt = p.path_times + 2 * (int64_t)pair * p.word_stride;
  int32_t* wt = p.word_times + 2 * (int64_t)pair * p.word_stride;
  int32_t* tok = p.tokens + 4 * (int64_t)pair * p.token_stride;
  int32_t* pho = p.phones ? p.phones + 3 * (int64_t)pair * p.phone_stride : nullptr;

  for (int k = tid; k < 2 * p.word_stride; k += kWaThreads) { pt[k] = -1; wt[k] = -1; }
  // ---- the path: arcs from the end state back to the start; every back-pointer is checked against the state's arcs ----
  if (tid == 0) {
    bool fail = p.bp_status[pair] != 0;
    int n = 0;
    for (int s = S - 1; s > 0 && !fail;) {
      const int a = bp[s];
      if (n >= depth || a < in_off[s] || a >= in_off[s + 1]) { fail = true; break; }
      path[n++] = a;
      s = src[a];
    }
    sh_na = n; sh_fail = fail;
  }
  __syncthreads();
  const int na = sh_na;
  if (sh_fail) {
    if (tid == 0) { p.status[pair] = 3; p.reason[pair] = 0; p.ntokens[pair] = 0; p.nphones[pair] = 0; }
    return;
  }
  // ---- begin frame of every arc = prefix sum of the string lengths; the word arcs' own times and labels ----
  I2 carry2 = I2{0, 0};
  for (int base = 0; base < na; base += kWaThreads) {
    const int j = base + tid;
    int len = 0, isw = 0, a = 0;
    if (j < na) { a = path[na - 1 - j]; len = (int)(tid_off[a + 1] - tid_off[a]); isw = word[a] != 0; }
    const I2 inc = wa_scan(I2{len, isw}, OpSum2(), carry2, sh_w2);
    if (j < na) {
      const int begin = inc.a - len, rank = inc.b - 1;
      pbeg[j] = begin;
      if (isw) {
        plab[rank] = word_ids[word[a]];
        if (rank < p.word_stride) { pt[2 * rank] = begin; pt[2 * rank + 1] = begin + len; }
      }
    }
  }
  const int T = min(carry2.a, fcap), m = carry2.b;
  __syncthreads();
  // ---- the path's string: one wavefront per arc, the lanes along the string ----
  for (int j = wave; j < na; j += kWaWaves) {
    const int a = path[na - 1 - j], b = pbeg[j];
    const int64_t o = tid_off[a];
    const int len = (int)(tid_off[a + 1] - o);
    for (int i = lane; i < len && b + i < T; i += 64) {
      const int2 e = p.tid_tab[p.tids[o + i]];
      fts[b + i] = e.x; fpf[b + i] = e.y;
    }
  }
  __syncthreads();
  // ---- SplitToPhones.  reordered: the first adjacent pair in one transition-state that differs in the self-loop flag ----
  int key = INT_MAX;
  for (int i = tid; i + 1 < T; i += kWaThreads)
    if (fts[i] == fts[i + 1] && ((fpf[i] ^ fpf[i + 1]) & 1)) key = min(key, 2 * i + (fpf[i] & 1));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
  if (lane == 0) sh_w[wave] = key;
  __syncthreads();
  key = sh_w[0];
#pragma unroll
  for (int w = 1; w < kWaWaves; ++w) key = min(key, sh_w[w]);
  const bool reordered = key == INT_MAX || !(key & 1);
  __syncthreads();
  int carry_m = -1, carry_c = 0, last_cut = 1, flags = 0;      // flags: 1 split not ok, 2 partial token, 8 phone without category
  for (int base = 0; base < T; base += kWaThreads) {
    const int i = base + tid;
    const bool valid = i < T, has_n = i + 1 < T;
    const int ts = valid ? fts[i] : 0, pf = valid ? fpf[i] : 0;
    const int ts_p = valid && i > 0 ? fts[i - 1] : 0, pf_p = valid && i > 0 ? fpf[i - 1] : 0;
    const int ts_n = has_n ? fts[i + 1] : 0, pf_n = has_n ? fpf[i + 1] : 0;
    const bool fin = (pf & 2) != 0;
    // absorbable: a self-loop in the transition-state of the frame before it, which a reordered model puts behind the
    // transition out of the state
    const bool ab = reordered && valid && i > 0 && (pf & 1) && ts == ts_p;
    const bool ab_n = reordered && has_n && (pf_n & 1) && ts_n == ts;
    // e: 2 i + fin for a frame that is not absorbable, 2 i + 1 for an absorbable one with fin; the running maximum is
    // odd exactly when a fin was seen since the last frame that is not absorbable (that frame included)
    const int e = !valid ? -1 : (!ab ? 2 * i + (fin ? 1 : 0) : (fin ? 2 * i + 1 : -1));
    const int m_before = carry_m;
    const int mi = wa_scan(e, OpMax(), carry_m, sh_w);
    sh_m[tid] = mi;
    __syncthreads();
    const int m_prev = tid > 0 ? sh_m[tid - 1] : m_before;
    const bool skipped = ab && m_prev >= 0 && (m_prev & 1), skipped_n = ab_n && mi >= 0 && (mi & 1);
    int cut = 0;
    if (valid) {
      if (skipped || fin) cut = !skipped_n;
      else if (!has_n || (ts != ts_n && (pf >> 2) != (pf_n >> 2))) { cut = 1; flags |= 1; }
    }
    sh_cut[tid] = cut;
    const int ci = wa_scan(cut, OpSum(), carry_c, sh_w);
    const int cut_prev = tid > 0 ? sh_cut[tid - 1] : last_cut;
    last_cut = sh_cut[kWaThreads - 1];
    if (valid) {
      if (cut_prev) { const int idx = ci - cut; php[idx] = pf >> 2; phb[idx] = i; }
      else if ((pf >> 2) != (pf_p >> 2)) flags |= 1;
    }
  }
  const int nph = carry_c;
  __syncthreads();
  // ---- tokens: word-boundary categories of the phones; words by rank ----
  I2 carry_s = I2{-1, 0}, carry_t = I2{0, 0};
  for (int base = 0; base < nph; base += kWaThreads) {
    const int k = base + tid;
    const bool valid = k < nph, has_n = k + 1 < nph;
    const int ph = valid ? php[k] : 0, b = valid ? phb[k] : 0, b_n = has_n ? phb[k + 1] : T;
    auto cat = [&](int q) { return q < p.num_phones ? (int)p.cat[q] : 255; };
    const int c = valid ? cat(ph) : 0, c_p = valid && k > 0 ? cat(php[k - 1]) : 0, c_n = has_n ? cat(php[k + 1]) : 0;
    const bool start = valid && (k == 0 || wa_starts_token(c) || wa_ends_token(c_p));
    const bool end = valid && (!has_n || wa_starts_token(c_n) || wa_ends_token(c));
    const int want = start ? (end ? -1 : 1) : (end ? 2 : 3);          // -1: alone in its token, nonword or singleton
    const bool bad = valid && (want < 0 ? (c != 0 && c != 4) : c != want);
    if (valid && c == 255) flags |= 8;
    const I2 seg = wa_scan(I2{start ? k : -1, bad ? 1 : 0}, OpSeg(), carry_s, sh_w2);
    const bool sil = end && seg.a == k && c == 0, wordb = end && !sil;
    const I2 cnt = wa_scan(I2{end ? 1 : 0, wordb ? 1 : 0}, OpSum2(), carry_t, sh_w2);
    if (valid && pho && k < p.phone_stride) { pho[3 * k] = ph; pho[3 * k + 1] = b; pho[3 * k + 2] = b_n - b; }
    if (end) {
      const int t = cnt.a - 1, rank = cnt.b - 1, begin = phb[seg.a];
      if (wordb && seg.b) flags |= 2;
      if (t < p.token_stride) {
        tok[4 * t] = wordb && rank < m ? plab[rank] : 0;
        tok[4 * t + 1] = begin; tok[4 * t + 2] = b_n - begin; tok[4 * t + 3] = sil ? 0 : (seg.b ? 2 : 1);
      }
      if (wordb && rank < m && rank < p.word_stride) { wt[2 * rank] = begin; wt[2 * rank + 1] = b_n; }
    }
  }
  int reason = (__syncthreads_or(flags & 1) ? 1 : 0) | (__syncthreads_or(flags & 2) ? 2 : 0) | (__syncthreads_or(flags & 8) ? 8 : 0);
  if (carry_t.b != m) reason |= 4;
  // malformed: the arcs' own times, so that a CTM can always be written (the barriers above made them visible)
  if (reason) for (int k = tid; k < 2 * min(m, p.word_stride); k += kWaThreads) wt[k] = pt[k];
  if (tid == 0) { p.status[pair] = reason ? 1 : 0; p.reason[pair] = reason; p.ntokens[pair] = carry_t.a; p.nphones[pair] = nph; }
}

bool wa_range_ok(const WordLat* h, int first, int count) { return h && first >= 0 && count >= 1 && (int64_t)first + count <= h->N; }

size_t wa_bytes(const WordLat* h, int first, int count, int G) {
  return (size_t)((h->align_pre[first + count] - h->align_pre[first]) * G) * 8;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" int pk2_wordlat_set_strings(void* handle, const int64_t* tid_off, const int32_t* tids) {
  WordLat* h = static_cast<WordLat*>(handle);
  PK2_REQUIRE(h && tid_off && tids, "wordlat_set_strings: null pointer");
  PK2_REQUIRE(h->N >= 1, "wordlat_set_strings: not a batch of pk2_wordlat_create");
  PK2_REQUIRE(!h->sblob, "wordlat_set_strings: the batch has its strings already");
  const int64_t TA = h->arc_off[h->N];
  PK2_REQUIRE(tid_off[0] == 0, "wordlat_set_strings: offsets must start at 0");
  for (int64_t a = 0; a < TA; ++a)
    PK2_REQUIRE(tid_off[a + 1] >= tid_off[a], "wordlat_set_strings: offsets decrease at arc %lld", (long long)a);
  const int64_t NT = tid_off[TA];
  int32_t max_tid = 0;
  for (int64_t i = 0; i < NT; ++i) {
    PK2_REQUIRE(tids[i] >= 1, "wordlat_set_strings: transition-id %d at position %lld (transition-ids start at 1)", tids[i], (long long)i);
    max_tid = std::max(max_tid, tids[i]);
  }
  // frame capacity: the longest start -> end path in frames.  Arcs are sorted by destination and every arc goes up a
  // level, so the arcs into a state come after all arcs into its predecessors.
  std::vector<int32_t> fcap(h->N);
  std::vector<int64_t> pre(h->N + 1, 0);
  for (int l = 0; l < h->N; ++l) {
    const int64_t S = h->state_off[l + 1] - h->state_off[l], a0 = h->arc_off[l], a1 = h->arc_off[l + 1];
    std::vector<int64_t> far(S, 0);
    for (int64_t a = a0; a < a1; ++a)
      far[h->h_dst[a]] = std::max(far[h->h_dst[a]], far[h->h_src[a]] + (tid_off[a + 1] - tid_off[a]));
    PK2_REQUIRE(far[S - 1] < (1 << 30), "wordlat_set_strings: lattice %d has a path of %lld frames", l, (long long)far[S - 1]);
    fcap[l] = (int32_t)far[S - 1];
    pre[l + 1] = pre[l] + (3 * (int64_t)h->depth[l] + 4 * (int64_t)fcap[l] + 1) / 2;
  }
  Carver sz(nullptr);
  auto carve = [&](Carver& c, WordLat* o) {
    o->d_tid_off = c.take<int64_t>(TA + 1); o->d_align_pre = c.take<int64_t>(h->N + 1);
    o->d_tids = c.take<int32_t>(NT); o->d_fcap = c.take<int32_t>(h->N);
  };
  WordLat dummy;
  carve(sz, &dummy);
  void* blob = nullptr;
  PK2_HIP(hipMalloc(&blob, sz.bytes()));
  Carver cv(blob);
  carve(cv, h);
  hipError_t e = hipMemcpy(const_cast<int64_t*>(h->d_tid_off), tid_off, 8 * (TA + 1), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(const_cast<int64_t*>(h->d_align_pre), pre.data(), 8 * (h->N + 1), hipMemcpyHostToDevice);
  if (e == hipSuccess && NT) e = hipMemcpy(const_cast<int32_t*>(h->d_tids), tids, 4 * NT, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(const_cast<int32_t*>(h->d_fcap), fcap.data(), 4 * h->N, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(blob);
    set_error("wordlat_set_strings: upload -> %s", hipGetErrorString(e));
    return PK2_ERR_HIP;
  }
  h->sblob = blob; h->fcap = fcap; h->align_pre = pre; h->max_tid = max_tid;
  return PK2_OK;
}

extern "C" int pk2_wordlat_frame_capacity(const void* handle, int32_t* out) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && out, "wordlat_frame_capacity: null pointer");
  PK2_REQUIRE(h->sblob, "wordlat_frame_capacity: no strings (pk2_wordlat_set_strings comes first)");
  for (int l = 0; l < h->N; ++l) out[l] = h->fcap[l];
  return PK2_OK;
}

extern "C" int pk2_wordalign_model_create(int32_t num_tids, const int32_t* tid_tstate, const int32_t* tid_phone,
                                          const uint8_t* tid_flags, int32_t num_phones, const uint8_t* phone_cat, void* stream,
                                          void** out) {
  PK2_REQUIRE(out, "wordalign_model_create: null output");
  *out = nullptr;
  PK2_REQUIRE(tid_tstate && tid_phone && tid_flags && phone_cat, "wordalign_model_create: null pointer");
  PK2_REQUIRE(num_tids >= 1 && num_phones >= 1, "wordalign_model_create: %d transition-ids, %d phones", num_tids, num_phones);
  std::vector<int2> tab(num_tids + 1);
  tab[0] = make_int2(0, 0);
  for (int32_t t = 1; t <= num_tids; ++t) {
    PK2_REQUIRE(tid_phone[t] >= 0 && tid_phone[t] < (1 << 29), "wordalign_model_create: phone %d of transition-id %d", tid_phone[t], t);
    tab[t] = make_int2(tid_tstate[t], tid_phone[t] << 2 | (tid_flags[t] & 3));
  }
  for (int32_t q = 0; q < num_phones; ++q)
    PK2_REQUIRE(phone_cat[q] <= 4 || phone_cat[q] == 255, "wordalign_model_create: category %d of phone %d", phone_cat[q], q);
  WordAlignModel* m = new WordAlignModel;
  m->num_tids = num_tids; m->num_phones = num_phones;
  Carver sz(nullptr);
  sz.take<int2>(num_tids + 1); sz.take<uint8_t>(num_phones);
  hipError_t e = hipMalloc(&m->blob, sz.bytes());
  if (e != hipSuccess) { delete m; set_error("wordalign_model_create: hipMalloc -> %s", hipGetErrorString(e)); return PK2_ERR_HIP; }
  Carver cv(m->blob);
  m->d_tid = cv.take<int2>(num_tids + 1); m->d_cat = cv.take<uint8_t>(num_phones);
  hipStream_t st = static_cast<hipStream_t>(stream);
  e = hipMemcpyAsync(const_cast<int2*>(m->d_tid), tab.data(), sizeof(int2) * (num_tids + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(const_cast<uint8_t*>(m->d_cat), phone_cat, num_phones, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(m->blob);
    delete m;
    set_error("wordalign_model_create: upload -> %s", hipGetErrorString(e));
    return PK2_ERR_HIP;
  }
  *out = m;
  return PK2_OK;
}

extern "C" int pk2_wordalign_model_destroy(void* model) {
  WordAlignModel* m = static_cast<WordAlignModel*>(model);
  if (!m) return PK2_OK;
  if (m->blob) PK2_HIP(hipFree(m->blob));
  delete m;
  return PK2_OK;
}

extern "C" size_t pk2_wordlat_align_workspace_bytes(const void* handle, int32_t first, int32_t count, int32_t G) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  if (!wa_range_ok(h, first, count) || !h->sblob || G < 1 || G > PK2_WORDLAT_MAX_SETTINGS) return 0;
  return wa_bytes(h, first, count, G);
}

extern "C" int pk2_wordlat_align_words(const void* handle, const void* model, int32_t first, int32_t count, int32_t G,
                                       const int32_t* backpointer, const int32_t* bp_status, void* work, size_t work_bytes,
                                       int32_t* path_times, int32_t* word_times, int32_t word_stride, int32_t* tokens,
                                       int32_t* ntokens, int32_t token_stride, int32_t* phones, int32_t* nphones,
                                       int32_t phone_stride, int32_t* status, int32_t* reason, void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  const WordAlignModel* m = static_cast<const WordAlignModel*>(model);
  PK2_REQUIRE(h && m && backpointer && bp_status && work && path_times && word_times && tokens && ntokens && nphones && status &&
              reason, "wordlat_align_words: null pointer");
  PK2_REQUIRE(h->sblob, "wordlat_align_words: no strings (pk2_wordlat_set_strings comes first)");
  PK2_REQUIRE(h->max_tid <= m->num_tids, "wordlat_align_words: the strings hold transition-id %d, the model has %d", h->max_tid,
              m->num_tids);
  PK2_REQUIRE(G >= 1 && G <= PK2_WORDLAT_MAX_SETTINGS, "wordlat_align_words: %d settings (1..%d)", G, PK2_WORDLAT_MAX_SETTINGS);
  PK2_REQUIRE(wa_range_ok(h, first, count), "wordlat_align_words: lattices %d..%d of %d", first, first + count, h->N);
  for (int l = first; l < first + count; ++l) {
    PK2_REQUIRE(word_stride >= h->depth[l], "wordlat_align_words: word_stride %d below the depth %d of lattice %d", word_stride,
                h->depth[l], l);
    PK2_REQUIRE(token_stride >= h->fcap[l] && phone_stride >= h->fcap[l],
                "wordlat_align_words: token_stride %d / phone_stride %d below the %d frames lattice %d can hold", token_stride,
                phone_stride, h->fcap[l], l);
  }
  PK2_REQUIRE(work_bytes >= wa_bytes(h, first, count, G) && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_align_words: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, wa_bytes(h, first, count, G));
  WaParams p;
  p.state_off = h->d_state_off; p.arc_off = h->d_arc_off; p.level_off_off = h->d_level_off_off; p.word_off_off = h->d_word_off_off;
  p.tid_off = h->d_tid_off; p.align_pre = h->d_align_pre; p.src = h->d_src; p.word = h->d_word; p.in_off = h->d_in_off;
  p.word_ids = h->d_word_ids; p.tids = h->d_tids; p.fcap = h->d_fcap; p.tid_tab = m->d_tid; p.cat = m->d_cat;
  p.num_phones = m->num_phones; p.first = first; p.G = G; p.bp = backpointer; p.bp_status = bp_status;
  p.work = static_cast<int32_t*>(work); p.path_times = path_times; p.word_times = word_times; p.tokens = tokens;
  p.ntokens = ntokens; p.phones = phones; p.nphones = nphones; p.status = status; p.reason = reason;
  p.word_stride = word_stride; p.token_stride = token_stride; p.phone_stride = phone_stride;
  hipLaunchKernelGGL(wa_kernel, dim3(count * G), dim3(kWaThreads), 0, static_cast<hipStream_t>(stream), p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
