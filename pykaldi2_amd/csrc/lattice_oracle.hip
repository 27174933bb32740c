// Lattice oracle (include/pk2hip.h: pk2_wordlat_oracle): the smallest edit distance between a reference and
// any path of a packed word lattice (Kaldi's lattice-oracle), the path that reaches it and the split into insertions,
// deletions and substitutions.  tests/oracle_ref.py states the recurrence and the tie rule; this file follows it.
//
//   ws_oracle_kernel   one workgroup of 1024 threads per lattice.  D (S x (R + 1), int32) lives in the caller's workspace,
//                      because an arc may skip levels and the walk back needs every row.  Levels in order with a barrier
//                      between them; inside a level one lane group per state (16 or 32 lanes while R + 1 fits, otherwise a
//                      wavefront over chunks of 64 positions): per incoming arc two coalesced loads (D[s][j], D[s][j-1]),
//                      the deletion chain as a prefix minimum of C - j over the lanes with a carry from chunk to chunk.  The
//                      end state's arcs (one per final state) are cut into one slice per lane group; the partial minima go
//                      through rows behind the table and the first group finishes the row.  Wavefront 0 walks back (64 arcs
//                      of a state tested at once, the lowest fitting arc taken), then all threads write the outputs.
//
// Integer arithmetic, minima only: no atomics, nothing depends on the launch geometry or on the order of the minima, so a
// lattice gives the same bytes alone, in a batch and in any launch split.
#include <vector>

#include "common.h"
#include "wordlat.h"

#pragma clang fp contract(off)

namespace pk2 {
namespace {

constexpr int kOrThreads = 1024;
constexpr int kOrPartRows = kOrThreads / 16;   // partial rows of the end state: one per lane group at the smallest width
constexpr int kOrInf = 0x3FFFFFFF;

// int32 cells of one lattice's area: [D S x P | partial rows kOrPartRows x P | path depth | labels depth], even (8 bytes).
__host__ __device__ inline int64_t or_cells(int64_t S, int64_t depth, int64_t R) {
  if (R < 0 || R > PK2_WORDLAT_MAX_POSITIONS) return 0;
  return ((S + kOrPartRows) * (R + 1) + 2 * depth + 1) & ~(int64_t)1;
}

struct OrParams {
  const int64_t *state_off, *arc_off, *level_off_off, *word_off_off, *ref_off;
  const int32_t *src, *in_off, *level_off, *word_ids, *label, *ref;
  int32_t first, count;
  int32_t* work; int64_t work_cells;
  int32_t *errors, *counts, *words, *nwords, *path, *npath, *status;
  int32_t word_stride, path_stride;
};

struct OrView {
  int S, A, depth, R, P;
  const int32_t *src, *in_off, *level_off, *word_ids, *label, *ref;
  int32_t *D, *part, *tarc, *tlab;
};

// C[n][j] over the arcs a0 .. a1 of one destination state, for the position j of this lane (j <= R).
__device__ __forceinline__ int or_arcs(const OrView& L, int a0, int a1, int j, int rl) {
  int best = kOrInf;
#pragma unroll 4
  for (int a = a0; a < a1; ++a) {
    const int lb = L.label[a];
    const int32_t* row = L.D + (int64_t)L.src[a] * L.P;
    const int up = row[j];
    int cand = up + (lb != 0 ? 1 : 0);
    if (lb != 0 && j >= 1) cand = min(cand, row[j - 1] + (lb != rl ? 1 : 0));
    best = min(best, cand);
  }
  return best;
}

// The deletion chain of one chunk: v = C - j in, D - j out; `carry` = the minimum over all earlier chunks.
template <int GW>
__device__ __forceinline__ int or_chain(int v, int gl, int& carry) {
#pragma unroll
  for (int o = 1; o < GW; o <<= 1) { const int u = __shfl_up(v, o, GW); if (gl >= o) v = min(v, u); }
  v = min(v, carry);
  carry = __shfl(v, GW - 1, GW);
  return v;
}

template <int GW>
__device__ __forceinline__ void or_levels(const OrView& L, int tid) {
  constexpr int NG = kOrThreads / GW;
  const int grp = tid / GW, gl = tid % GW, nc = L.R / GW + 1;
  for (int lev = 1; lev < L.depth; ++lev) {
    for (int s = L.level_off[lev] + grp; s < L.level_off[lev + 1]; s += NG) {
      const int a0 = L.in_off[s], a1 = L.in_off[s + 1];
      int32_t* out = L.D + (int64_t)s * L.P;
      int carry = kOrInf;
      for (int c = 0; c < nc; ++c) {
        const int j = GW * c + gl;
        const bool in = j <= L.R;
        const int rl = (in && j >= 1) ? L.ref[j - 1] : 0;
        const int cm = in ? or_arcs(L, a0, a1, j, rl) : kOrInf;
        const int v = or_chain<GW>(cm - j, gl, carry);
        if (in) out[j] = v + j;
      }
    }
    __syncthreads();
  }
  // the end state: a contiguous slice of its arcs per lane group, then the first group takes the minimum over the slices
  const int e0 = L.in_off[L.S - 1], n = L.A - e0, per = (n + NG - 1) / NG, used = (n + per - 1) / per;
  if (grp < used) {
    const int a0 = e0 + grp * per, a1 = min(L.A, a0 + per);
    for (int c = 0; c < nc; ++c) {
      const int j = GW * c + gl;
      if (j <= L.R) L.part[(int64_t)grp * L.P + j] = or_arcs(L, a0, a1, j, j >= 1 ? L.ref[j - 1] : 0);
    }
  }
  __syncthreads();
  if (grp == 0) {
    int32_t* out = L.D + (int64_t)(L.S - 1) * L.P;
    int carry = kOrInf;
    for (int c = 0; c < nc; ++c) {
      const int j = GW * c + gl;
      const bool in = j <= L.R;
      int cm = kOrInf;
      if (in) for (int g = 0; g < used; ++g) cm = min(cm, L.part[(int64_t)g * L.P + j]);
      const int v = or_chain<GW>(cm - j, gl, carry);
      if (in) out[j] = v + j;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kOrThreads) ws_oracle_kernel(OrParams p) {
  const int li = blockIdx.x, l = p.first + li, tid = threadIdx.x, lane = tid & 63;
  __shared__ long long sh_sum[kOrThreads];
  __shared__ int sh_res[8];
  // where this lattice's area begins: the cells of the lattices before it in the range
  long long before = 0;
  for (int k = tid; k < li; k += kOrThreads) {
    const int m = p.first + k;
    before += or_cells(p.state_off[m + 1] - p.state_off[m], p.level_off_off[m + 1] - p.level_off_off[m] - 2,
                       p.ref_off[k + 1] - p.ref_off[k]);
  }
  sh_sum[tid] = before;
  __syncthreads();
  for (int o = kOrThreads / 2; o > 0; o >>= 1) {
    if (tid < o) sh_sum[tid] += sh_sum[tid + o];
    __syncthreads();
  }
  before = sh_sum[0];
  OrView L;
  const int64_t so = p.state_off[l], ao = p.arc_off[l], lo = p.level_off_off[l], wo = p.word_off_off[l];
  const int64_t R64 = p.ref_off[li + 1] - p.ref_off[li];
  L.S = (int)(p.state_off[l + 1] - so);
  L.A = (int)(p.arc_off[l + 1] - ao);
  L.depth = (int)(p.level_off_off[l + 1] - lo) - 2;
  L.src = p.src + ao; L.label = p.label + ao;
  L.in_off = p.in_off + so + l;
  L.level_off = p.level_off + lo;
  L.word_ids = p.word_ids + wo - l;
  L.ref = p.ref + p.ref_off[li];
  int32_t* wrow = p.words + (int64_t)li * p.word_stride;
  int32_t* prow = p.path + (int64_t)li * p.path_stride;
  const int64_t cells = or_cells(L.S, L.depth, R64);
  // a reference beyond the capacity, or offsets that do not agree with the ones the workspace was sized from
  if (R64 < 0 || R64 > PK2_WORDLAT_MAX_POSITIONS || before + cells > p.work_cells) {
    for (int i = tid; i < p.word_stride; i += kOrThreads) wrow[i] = -1;
    for (int i = tid; i < p.path_stride; i += kOrThreads) prow[i] = -1;
    if (tid == 0) { p.errors[li] = -1; p.status[li] = (R64 > PK2_WORDLAT_MAX_POSITIONS) ? 2 : 3; }
    return;
  }
  L.R = (int)R64; L.P = L.R + 1;
  L.D = p.work + before;
  L.part = L.D + (int64_t)L.S * L.P;
  L.tarc = L.part + (int64_t)kOrPartRows * L.P;
  L.tlab = L.tarc + L.depth;
  for (int j = tid; j <= L.R; j += kOrThreads) L.D[j] = j;
  __syncthreads();
  if (L.P <= 16) or_levels<16>(L, tid);
  else if (L.P <= 32) or_levels<32>(L, tid);
  else or_levels<64>(L, tid);
  // ---- the walk back (wavefront 0): the lowest incoming arc that fits, its edit type in the order diagonal, free,
  // insertion; a deletion if no arc fits ----
  if (tid < 64) {
    int n = L.S - 1, j = L.R, np = 0, nw = 0, nins = 0, ndel = 0, nsub = 0, steps = 0;
    bool ok = true;
    while (ok && (n != 0 || j != 0)) {
      if (++steps > L.depth + L.R + 1) { ok = false; break; }
      const int cur = L.D[(int64_t)n * L.P + j];
      const int a0 = L.in_off[n], a1 = L.in_off[n + 1];
      const int rl = j >= 1 ? L.ref[j - 1] : 0;
      bool found = false;
      int t = 0, u = 0, lb = 0, arc = 0;
      for (int base = a0; base < a1 && !found; base += 64) {
        const int a = base + lane;
        t = 0;
        if (a < a1) {
          u = L.src[a]; lb = L.label[a];
          const int32_t* row = L.D + (int64_t)u * L.P;
          if (lb != 0) {
            if (j >= 1 && row[j - 1] + (lb != rl ? 1 : 0) == cur) t = lb != rl ? 2 : 1;
            else if (row[j] + 1 == cur) t = 3;
          } else if (row[j] == cur) {
            t = 4;
          }
        }
        const unsigned long long mask = __ballot(t != 0);
        if (mask != 0) {
          const int f = __ffsll((long long)mask) - 1;
          t = __shfl(t, f, 64); u = __shfl(u, f, 64); lb = __shfl(lb, f, 64);
          arc = base + f;
          found = true;
        }
      }
      if (found) {
        if (np >= L.depth) { ok = false; break; }
        if (lane == 0) { L.tarc[np] = arc; if (lb != 0) L.tlab[nw] = lb; }
        ++np;
        nw += lb != 0;
        nsub += t == 2;
        nins += t == 3;
        if (t == 1 || t == 2) --j;
        n = u;
      } else {
        if (j < 1 || L.D[(int64_t)n * L.P + j - 1] + 1 != cur) { ok = false; break; }
        ++ndel;
        --j;
      }
    }
    if (lane == 0) {
      const int e = L.D[(int64_t)(L.S - 1) * L.P + L.R];
      ok = ok && nins + ndel + nsub == e;
      sh_res[0] = ok ? np : 0; sh_res[1] = ok ? nw : 0;
      p.errors[li] = ok ? e : -1;
      p.status[li] = ok ? 0 : 3;
      if (ok) {
        p.counts[3 * (int64_t)li] = nins; p.counts[3 * (int64_t)li + 1] = ndel; p.counts[3 * (int64_t)li + 2] = nsub;
        p.nwords[li] = nw; p.npath[li] = np;
      }
    }
  }
  __syncthreads();
  const int np = sh_res[0], nw = sh_res[1];
  for (int i = tid; i < p.word_stride; i += kOrThreads) wrow[i] = i < nw ? L.word_ids[L.tlab[nw - 1 - i]] : -1;
  for (int i = tid; i < p.path_stride; i += kOrThreads) prow[i] = i < np ? L.tarc[np - 1 - i] : -1;
}

bool or_range_ok(const WordLat* h, int first, int count) {
  return h && first >= 0 && count >= 1 && (int64_t)first + count <= h->N;
}

bool or_offsets_ok(const int64_t* ref_off, int count) {
  if (!ref_off || ref_off[0] < 0) return false;
  for (int i = 0; i < count; ++i) if (ref_off[i + 1] < ref_off[i]) return false;
  return true;
}

int64_t or_total_cells(const WordLat* h, int first, int count, const int64_t* ref_off) {
  int64_t w = 0;
  for (int i = 0; i < count; ++i) {
    const int l = first + i;
    w += or_cells(h->state_off[l + 1] - h->state_off[l], h->depth[l], ref_off[i + 1] - ref_off[i]);
  }
  return w;
}

}  // namespace
}  // namespace pk2

using namespace pk2;

extern "C" size_t pk2_wordlat_oracle_workspace_bytes(const void* handle, int32_t first, int32_t count, const int64_t* ref_off) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  if (!or_range_ok(h, first, count) || !or_offsets_ok(ref_off, count)) return 0;
  return (size_t)or_total_cells(h, first, count, ref_off) * 4 + 8;
}

extern "C" int pk2_wordlat_oracle(const void* handle, int32_t first, int32_t count, const int32_t* arc_label, const int32_t* ref,
                                  const int64_t* ref_off, const int64_t* ref_off_host, void* work, size_t work_bytes,
                                  int32_t* errors, int32_t* counts, int32_t* words, int32_t word_stride, int32_t* nwords,
                                  int32_t* path, int32_t path_stride, int32_t* npath, int32_t* status, void* stream) {
  const WordLat* h = static_cast<const WordLat*>(handle);
  PK2_REQUIRE(h && arc_label && ref && ref_off && ref_off_host && work && errors && counts && words && nwords && path && npath &&
              status, "wordlat_oracle: null pointer");
  PK2_REQUIRE(or_range_ok(h, first, count), "wordlat_oracle: lattices %d..%d of %d", first, first + count, h->N);
  PK2_REQUIRE(or_offsets_ok(ref_off_host, count), "wordlat_oracle: ref_off must start at >= 0 and never decrease");
  for (int l = first; l < first + count; ++l) {
    PK2_REQUIRE(word_stride >= h->depth[l], "wordlat_oracle: word_stride %d below the depth %d of lattice %d", word_stride,
                h->depth[l], l);
    PK2_REQUIRE(path_stride >= h->depth[l], "wordlat_oracle: path_stride %d below the depth %d of lattice %d", path_stride,
                h->depth[l], l);
  }
  const int64_t cells = or_total_cells(h, first, count, ref_off_host);
  PK2_REQUIRE(work_bytes >= (size_t)cells * 4 + 8 && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
              "wordlat_oracle: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, (size_t)cells * 4 + 8);
  OrParams p;
  memset(&p, 0, sizeof(p));
  p.state_off = h->d_state_off; p.arc_off = h->d_arc_off; p.level_off_off = h->d_level_off_off; p.word_off_off = h->d_word_off_off;
  p.ref_off = ref_off; p.src = h->d_src; p.in_off = h->d_in_off; p.level_off = h->d_level_off; p.word_ids = h->d_word_ids;
  p.label = arc_label; p.ref = ref;
  p.first = first; p.count = count; p.work = static_cast<int32_t*>(work); p.work_cells = cells;
  p.errors = errors; p.counts = counts; p.words = words; p.nwords = nwords; p.path = path; p.npath = npath; p.status = status;
  p.word_stride = word_stride; p.path_stride = path_stride;
  hipLaunchKernelGGL(ws_oracle_kernel, dim3(count), dim3(kOrThreads), 0, static_cast<hipStream_t>(stream), p);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
