// Transducer (RNN-T) loss and gradient with an ADDITIVE joint on gfx950, fused: the [T][U+1][V] joint and its gradient are
// never stored (k2's rnnt_loss_simple).  With z[t,u,v] = am[t,v] + lm[u,v], ma_t / ml_u the row maxima,
// Ea = exp(am - ma), El = exp(lm - ml):
//
//   S[t,u]  = sum_v Ea[t,v] El[u,v]                 lse[t,u] = log S[t,u] + ma_t + ml_u
//   py[t,u] = am[t,b] + lm[u,b] - lse[t,u]          px[t,u] = am[t,l_{u+1}] + lm[u,l_{u+1}] - lse[t,u]
//   alpha / beta over the T x (U+1) grid, log p = alpha[T-1,U] + py[T-1,U]
//   G[t,u]  = (occ_x + occ_y)[t,u] / S[t,u]
//   grad_am = w (Ea o (G El)) - blank / label terms      grad_lm = w (El o (G^T Ea)) - blank / label terms
//
// Seven launches on one stream, none waits on another workgroup, nothing is read back, no float atomics:
//   td_rows     a wave per row of am and of lm: the row maximum (16-byte loads, scalar head and tail), the blank column, and
//               for an am row the label terms zl[t,u] = am[t,l_{u+1}] + lm[u,l_{u+1}].
//   td_product  the three matrix products on v_mfma_f32_32x32x2_f32, one kernel body: a workgroup of four waves owns a
//               64 x 64 output tile (a wave a 32 x 32 quarter), K runs in tiles of 32 in ascending order into ONE accumulator
//               (a fixed summation order; a K tile in float32, the tiles added up in float64).  The operands are staged into LDS k-major ([k][64], pitch 65) and the exponentials
//               are formed THERE, from the raw logits: there is no Ea / El buffer.  The next K tile is fetched into registers
//               while the current one is multiplied.  Rows, columns and k beyond the utterance's own T, U+1, V are staged as
//               zeros without touching memory.  Epilogues: normaliser -> S, px, py; gradients -> times Ea / El and w.
//   td_lattice  two workgroups per utterance: alpha from (0,0), beta from (T-1,U), along the anti-diagonals d = t + u in ONE
//               launch each.  A lane owns ONE grid column u; its cell on diagonal d needs its own value of diagonal d -+ 1
//               and one neighbour's: one __shfl_up / __shfl_down, across a wave boundary one LDS word per wave,
//               double-buffered: one barrier per diagonal.  px / py of the next diagonal are loaded ahead of the barrier.
//               The state is float64 in the LOG domain (DESIGN.md 7.21 says why not the scaled probabilities of ctc_chains).
//   td_occ      per cell occ_y, occ_x and G from alpha, beta, px, py, S and log p.
//   td_fix      a wave per row of either gradient: the blank term, and ONE lane per distinct label adds its positions in the
//               sorted order of the packed descriptor (repeated labels add deterministically).
// and td_greedy (pk2_transducer_greedy): a wave per utterance, greedy decoding with a table predictor.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.h"
#include "transducer_layout.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 64;             // output tile edge of td_product (a wave: 32 x 32)
constexpr int kTK = 32;               // K tile
constexpr int kPitch = kTile + 1;     // LDS row pitch of a staged [k][64] operand
constexpr int kMmThreads = 256;

using namespace pk2td;      // TdDesc, TdLayout, td_layout, td_base: shared with csrc/transducer_pruned.hip

// The logits of both operands and where their gradients go: row r of utterance n at [n * seq + r * row].
struct TdTensors {
  const float* am; int64_t am_seq, am_row;
  const float* lm; int64_t lm_seq, lm_row;
  float* gam; int64_t gam_seq, gam_row;
  float* glm; int64_t glm_seq, glm_row;
  int32_t Tpad, Upad1, V, blank;
};

// ---- td_rows: grid (blocks, N), a wave per row: am rows 0..T-1, then lm rows 0..U.
__global__ __launch_bounds__(256) void td_rows(const int32_t* __restrict__ pk, TdTensors p, float* __restrict__ ws) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U = d.U, U1 = U + 1, V = p.V;
  const TdLayout l = td_layout(T, U);
  float* base = ws + td_base(desc, n);
  const int32_t* lab = pk + d.lab;
  const float* am = p.am + (int64_t)n * p.am_seq;
  const float* lm = p.lm + (int64_t)n * p.lm_seq;
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int32_t*>(base + l.lp)[2] = 0;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (int r = wave; r < T + U1; r += nwaves) {
    const bool is_am = r < T;
    const float* row = is_am ? am + (int64_t)r * p.am_row : lm + (int64_t)(r - T) * p.lm_row;
    // the row as [head scalars][16-byte aligned float4s][tail scalars]; the scalars are at most 6, one lane each
    const int head = min(V, (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) >> 2));
    const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
    float m = -INFINITY;
    for (int v = lane; v < nvec; v += 64) {
      const float4 q = *reinterpret_cast<const float4*>(row + head + 4 * v);
      m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    }
    if (lane < head + V - tail0) m = fmaxf(m, row[lane < head ? lane : tail0 + lane - head]);
    m = pk2::wave_max(m);
    if (lane == 0) {
      (base + (is_am ? l.ma : l.ml))[is_am ? r : r - T] = m;
      (base + (is_am ? l.amb : l.lmb))[is_am ? r : r - T] = row[p.blank];
    }
    if (is_am)
      for (int u = lane; u < U; u += 64) (base + l.zl)[(size_t)r * U1 + u] = row[lab[u]] + lm[(int64_t)u * p.lm_row + lab[u]];
  }
}

// ---- td_product: C[64 x 64] = A[64 x K] B[K x 64] of one workgroup.  la(i, k) / lb(k, j): the operand values of tile row i /
// tile column j at k (0 outside the utterance, WITHOUT a load).  AK / BK: the operand is contiguous along k in memory (threads
// then walk k fastest when staging, so that the loads coalesce); otherwise along its row / column index.
// A K tile is summed by the matrix instruction in float32 from zero, the K tiles are added up in float64: a float32 sum over
// 1024 grid columns alone misses the gradients' 1e-4 (measured: 4.0e-4 on grad_am at T = 2, U = 1023).
struct TdAcc { double v[16]; };
template <bool AK, bool BK, class LA, class LB>
__device__ __forceinline__ TdAcc td_tile_mm(float* As, float* Bs, int K, LA la, LB lb) {
  const int tx = threadIdx.x, lane = tx & 63, wave = tx >> 6, hi = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  constexpr int kPer = kTile * kTK / kMmThreads;      // 8 values of either operand per thread
  float ra[kPer], rb[kPer];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int e = tx + kMmThreads * r;
      ra[r] = AK ? la(e >> 5, k0 + (e & 31)) : la(e & 63, k0 + (e >> 6));
      rb[r] = BK ? lb(k0 + (e & 31), e >> 5) : lb(k0 + (e >> 6), e & 63);
    }
  };
  TdAcc tot;
#pragma unroll
  for (int j = 0; j < 16; ++j) tot.v[j] = 0.0;
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kTK) {
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int e = tx + kMmThreads * r;
      As[AK ? (e & 31) * kPitch + (e >> 5) : (e >> 6) * kPitch + (e & 63)] = ra[r];
      Bs[BK ? (e & 31) * kPitch + (e >> 5) : (e >> 6) * kPitch + (e & 63)] = rb[r];
    }
    __syncthreads();
    if (k0 + kTK < K) fetch(k0 + kTK);
    // v_mfma_f32_32x32x2_f32: the lanes' half hi supplies k = hi of both operands
    const float* a = As + hi * kPitch + wm * 32 + l31;
    const float* b = Bs + hi * kPitch + wn * 32 + l31;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
    for (int kk = 0; kk < kTK / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk * kPitch], b[2 * kk * kPitch], acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) tot.v[j] += (double)acc[j];
    __syncthreads();
  }
  return tot;
}
// accumulator register j of a lane: tile row / column
__device__ __forceinline__ int td_acc_row(int j) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return (wave >> 1) * 32 + (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5);
}
__device__ __forceinline__ int td_acc_col() { return ((threadIdx.x >> 6) & 1) * 32 + (threadIdx.x & 31); }

// mode 0: S = Ea El^T and its epilogue, grid (ceil(U1max / 64), ceil(Tmax / 64), N)
// mode 1: grad_am = w Ea o (G El),      grid (ceil(V / 64), ceil(Tpad / 64), N)
// mode 2: grad_lm = w El o (G^T Ea),    grid (ceil(V / 64), ceil(Upad1 / 64), N)
template <int kMode>
__global__ __launch_bounds__(kMmThreads) void td_product(const int32_t* __restrict__ pk, TdTensors p, float* __restrict__ ws,
                                                         const int32_t* __restrict__ status) {
  __shared__ float As[kTK * kPitch], Bs[kTK * kPitch];
  const int n = blockIdx.z, m0 = blockIdx.y * kTile, n0 = blockIdx.x * kTile;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U1 = d.U + 1, V = p.V;
  const TdLayout l = td_layout(T, d.U);
  float* base = ws + td_base(desc, n);
  const float* am = p.am + (int64_t)n * p.am_seq;
  const float* lm = p.lm + (int64_t)n * p.lm_seq;
  const float* ma = base + l.ma;
  const float* ml = base + l.ml;
  const float* G = base + l.G;
  const int am_row = p.am_row, lm_row = p.lm_row;      // (the tensors of one utterance are below 2^31 floats: checked on the host)
  auto ea = [&](int t, int v) { return t < T && v < V ? __expf(am[(int64_t)t * am_row + v] - ma[t]) : 0.f; };
  auto el = [&](int u, int v) { return u < U1 && v < V ? __expf(lm[(int64_t)u * lm_row + v] - ml[u]) : 0.f; };
  if (kMode == 0) {
    if (m0 >= T || n0 >= U1) return;
    const TdAcc acc = td_tile_mm<true, true>(As, Bs, V, [&](int i, int k) { return ea(m0 + i, k); }, [&](int k, int j) { return el(n0 + j, k); });
    const int u = n0 + td_acc_col();
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int t = m0 + td_acc_row(j);
      if (t < T && u < U1) {
        const float s = (float)acc.v[j];
        bad = bad || !(s >= FLT_MIN && s < INFINITY);
        const double lse = log(acc.v[j]) + (double)ma[t] + (double)ml[u];
        const size_t c = (size_t)t * U1 + u;
        (base + l.S)[c] = s;
        (base + l.py)[c] = (float)(((double)(base + l.amb)[t] + (double)(base + l.lmb)[u]) - lse);
        (base + l.px)[c] = u < d.U ? (float)((double)(base + l.zl)[c] - lse) : 0.f;
      }
    }
    if (bad) reinterpret_cast<int32_t*>(base + l.lp)[2] = 1;      // (every writer writes the same 1)
  } else {
    const int rows = kMode == 1 ? T : U1, rows_pad = kMode == 1 ? p.Tpad : p.Upad1;
    float* g = kMode == 1 ? p.gam + (int64_t)n * p.gam_seq : p.glm + (int64_t)n * p.glm_seq;
    const int64_t g_row = kMode == 1 ? p.gam_row : p.glm_row;
    const int v = n0 + td_acc_col();
    if (status[n] != PK2_TRANSDUCER_OK || m0 >= rows) {      // every row of the tensor is written
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int r = m0 + td_acc_row(j);
        if (r < rows_pad && v < V) g[r * g_row + v] = 0.f;
      }
      return;
    }
    TdAcc acc;
    if (kMode == 1)
      acc = td_tile_mm<true, false>(As, Bs, U1, [&](int i, int k) { return m0 + i < T && k < U1 ? G[(size_t)(m0 + i) * U1 + k] : 0.f; },
                                    [&](int k, int j) { return el(k, n0 + j); });
    else
      acc = td_tile_mm<false, false>(As, Bs, T, [&](int i, int k) { return m0 + i < U1 && k < T ? G[(size_t)k * U1 + m0 + i] : 0.f; },
                                     [&](int k, int j) { return ea(k, n0 + j); });
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = m0 + td_acc_row(j);
      if (r < rows_pad && v < V) g[r * g_row + v] = r < rows ? (float)((double)d.w * ((double)(kMode == 1 ? ea(r, v) : el(r, v)) * acc.v[j])) : 0.f;
    }
  }
}

// ---- td_lattice: grid (2, N), blockDim = the batch's largest U + 1 rounded up to whole waves (a lane's arithmetic does not
// depend on it).  blockIdx.x = 0: alpha, loss and status; 1: beta.
__global__ __launch_bounds__(1024) void td_lattice(const int32_t* __restrict__ pk, float* __restrict__ ws, double* __restrict__ loss,
                                                   int32_t* __restrict__ status) {
  __shared__ double bnd[2][16];      // the value a wave hands to its neighbour wave
  const int n = blockIdx.y, u = threadIdx.x, lane = u & 63, wave = u >> 6, nw = blockDim.x >> 6;
  const bool fwd = blockIdx.x == 0;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U = d.U, U1 = U + 1, D = T + U;      // diagonals 0 .. D-1
  const TdLayout l = td_layout(T, U);
  float* base = ws + td_base(desc, n);
  const float* px = base + l.px;
  const float* py = base + l.py;
  const double NEG = -INFINITY;
  float xn = 0.f, yn = 0.f;            // px / py of this lane's cell on the next diagonal
  auto load = [&](int t) {
    if (u < U1 && t >= 0 && t < T) { xn = px[(size_t)t * U1 + u]; yn = py[(size_t)t * U1 + u]; }
  };
  if (fwd) {
    double* al = reinterpret_cast<double*>(base + l.al);
    double up = NEG, right = NEG, a = NEG;      // up: alpha + py of the own cell of the last diagonal, right: alpha + px of it
    load(-u);
    for (int dg = 0; dg < D; ++dg) {
      const int t = dg - u;
      const float xc = xn, yc = yn;
      load(t + 1);
      double left = __shfl_up(right, 1, 64);
      if (lane == 0) left = (wave > 0 && dg > 0) ? bnd[(dg - 1) & 1][wave - 1] : NEG;
      if (u < U1 && t >= 0 && t < T) {
        a = dg == 0 ? 0.0 : pk2::log_add(up, left);
        al[(size_t)t * U1 + u] = a;
        up = a + (double)yc;
        right = u < U ? a + (double)xc : NEG;
      } else {
        right = NEG;
      }
      if (lane == 63) bnd[dg & 1][wave] = right;
      __syncthreads();
    }
    if (u == U) {      // its last cell was (T-1, U): up = alpha[T-1, U] + py[T-1, U]
      const int32_t flag = reinterpret_cast<const int32_t*>(base + l.lp)[2];
      const bool ok = flag == 0 && up == up && up > -INFINITY && up < INFINITY;
      *reinterpret_cast<double*>(base + l.lp) = up;
      loss[n] = ok ? -up : 0.0;
      status[n] = ok ? PK2_TRANSDUCER_OK : PK2_TRANSDUCER_NUMERIC;
    }
  } else {
    double* be = reinterpret_cast<double*>(base + l.be);
    double b = NEG;
    load(D - 1 - u);
    for (int dg = D - 1; dg >= 0; --dg) {
      const int t = dg - u;
      const float xc = xn, yc = yn;
      load(t - 1);
      double right = __shfl_down(b, 1, 64);
      if (lane == 63) right = (wave + 1 < nw && dg < D - 1) ? bnd[(dg + 1) & 1][wave + 1] : NEG;
      if (u < U1 && t >= 0 && t < T) {
        const double below = t == T - 1 ? (u == U ? 0.0 : NEG) : b;      // beta[t+1, u]
        b = pk2::log_add((double)yc + below, u < U ? (double)xc + right : NEG);
        be[(size_t)t * U1 + u] = b;
      } else {
        b = NEG;
      }
      if (lane == 0) bnd[dg & 1][wave] = b;
      __syncthreads();
    }
  }
}

// ---- td_occ: grid (blocks, N), a thread per grid cell.
__global__ __launch_bounds__(256) void td_occ(const int32_t* __restrict__ pk, float* __restrict__ ws, const int32_t* __restrict__ status) {
  const int n = blockIdx.y;
  if (status[n] != PK2_TRANSDUCER_OK) return;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U = d.U, U1 = U + 1;
  const TdLayout l = td_layout(T, U);
  float* base = ws + td_base(desc, n);
  const double* al = reinterpret_cast<const double*>(base + l.al);
  const double* be = reinterpret_cast<const double*>(base + l.be);
  const double lp = *reinterpret_cast<const double*>(base + l.lp);
  const size_t C = (size_t)T * U1;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < C; c += (size_t)gridDim.x * blockDim.x) {
    const int t = (int)(c / U1), u = (int)(c % U1);
    const double a = al[c] - lp;
    const double by = t + 1 < T ? be[c + U1] : (u == U ? 0.0 : -INFINITY);
    const float oy = (float)exp(a + (double)(base + l.py)[c] + by);
    const float ox = u < U ? (float)exp(a + (double)(base + l.px)[c] + be[c + 1]) : 0.f;
    (base + l.oy)[c] = oy;
    (base + l.ox)[c] = ox;
    (base + l.G)[c] = (ox + oy) / (base + l.S)[c];
  }
}

// ---- td_fix: grid (Tmax + U1max, N), one wave: the terms of the gradients that are not a product.
__global__ __launch_bounds__(64) void td_fix(const int32_t* __restrict__ pk, TdTensors p, const float* __restrict__ ws,
                                             const int32_t* __restrict__ status, int32_t Tmax) {
  const int n = blockIdx.y, lane = threadIdx.x;
  if (status[n] != PK2_TRANSDUCER_OK) return;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U = d.U, U1 = U + 1;
  const TdLayout l = td_layout(T, U);
  const float* base = ws + td_base(desc, n);
  const float* oy = base + l.oy;
  const float* ox = base + l.ox;
  if ((int)blockIdx.x < Tmax) {
    const int t = blockIdx.x;
    if (t >= T) return;
    float* grow = p.gam + (int64_t)n * p.gam_seq + (int64_t)t * p.gam_row;
    double sy = 0.0;
    for (int u = lane; u < U1; u += 64) sy += (double)oy[(size_t)t * U1 + u];
    sy = pk2::wave_sum_d(sy);
    if (lane == 0) grow[p.blank] = (float)((double)grow[p.blank] - (double)d.w * sy);
    const int32_t* ord = pk + d.ord;
    const int32_t* slab = ord + U;
    for (int r = lane; r < U; r += 64) {
      const int32_t c = slab[r];
      if (r > 0 && slab[r - 1] == c) continue;      // the first slot of a label adds the whole group, in sorted order
      double acc = 0.0;
      for (int k = r; k < U && slab[k] == c; ++k) acc += (double)ox[(size_t)t * U1 + ord[k]];
      grow[c] = (float)((double)grow[c] - (double)d.w * acc);
    }
  } else {
    const int u = blockIdx.x - Tmax;
    if (u >= U1) return;
    float* grow = p.glm + (int64_t)n * p.glm_seq + (int64_t)u * p.glm_row;
    double sy = 0.0, sx = 0.0;
    for (int t = lane; t < T; t += 64) {
      sy += (double)oy[(size_t)t * U1 + u];
      sx += (double)ox[(size_t)t * U1 + u];
    }
    sy = pk2::wave_sum_d(sy);
    sx = pk2::wave_sum_d(sx);
    if (lane == 0) {
      grow[p.blank] = (float)((double)grow[p.blank] - (double)d.w * sy);
      if (u < U) {
        float* q = grow + (pk + d.lab)[u];
        *q = (float)((double)*q - (double)d.w * sx);
      }
    }
  }
}

// ---- td_greedy: grid N, one wave.  The sum am + table is a float32 sum; ties go to the lower column.
__global__ __launch_bounds__(64) void td_greedy(const int32_t* __restrict__ lengths, const float* __restrict__ am, int64_t seq_stride,
                                                int64_t frame_stride, const float* __restrict__ table, int64_t table_stride, int32_t V,
                                                int32_t blank, int32_t max_symbols, int32_t cap, int32_t* __restrict__ tokens,
                                                int32_t* __restrict__ lens) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int T = lengths[n];
  int32_t* out = tokens + (int64_t)n * cap;
  int prev = blank, count = 0;
  for (int t = 0; t < T; ++t) {
    const float* row = am + (int64_t)n * seq_stride + (int64_t)t * frame_stride;
    for (int s = 0; s < max_symbols; ++s) {
      const float* trow = table + (int64_t)prev * table_stride;
      float best = -INFINITY;
      int arg = V;
      for (int v = lane; v < V; v += 64) {
        const float z = row[v] + trow[v];
        if (z > best || arg == V) { best = z; arg = v; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa < V && (arg == V || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
      }
      if (arg == blank) break;
      if (lane == 0) out[count] = arg;
      ++count;
      prev = arg;
    }
  }
  for (int i = count + lane; i < cap; i += 64) out[i] = -1;
  if (lane == 0) lens[n] = count;
}

// Host-side check of the packed descriptor: everything a kernel indexes with is verified here, against the host copy.
int td_check(const int32_t* pk, int64_t words, int32_t N, int32_t Tpad, int32_t Upad1, int32_t V, int32_t blank, size_t* ws_words,
             int32_t* Tmax, int32_t* Umax) {
  PK2_REQUIRE(pk && N >= 1 && words >= (int64_t)N * 8, "transducer: descriptor of %lld words for %d utterances", (long long)words, N);
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  *ws_words = 0; *Tmax = 0; *Umax = 0;
  for (int32_t n = 0; n < N; ++n) {
    const TdDesc& d = desc[n];
    PK2_REQUIRE(d.T >= 1 && d.T <= Tpad, "transducer: utterance %d has %d frames, the tensor %d", n, d.T, Tpad);
    if (d.U < 0 || d.U > PK2_TRANSDUCER_MAX_LABELS) {
      pk2::set_error("transducer: utterance %d has %d labels (limit %d)", n, d.U, PK2_TRANSDUCER_MAX_LABELS);
      return PK2_ERR_LIMIT;
    }
    PK2_REQUIRE(d.U + 1 <= Upad1, "transducer: utterance %d needs %d predictor rows, the tensor has %d", n, d.U + 1, Upad1);
    PK2_REQUIRE(d.status == PK2_TRANSDUCER_OK, "transducer: utterance %d: status %d", n, d.status);
    PK2_REQUIRE(d.lab >= N * 8 && d.ord >= N * 8 && (int64_t)d.lab + d.U <= words && (int64_t)d.ord + 2 * (int64_t)d.U <= words,
                "transducer: utterance %d: label arrays outside the descriptor", n);
    const int32_t* lab = pk + d.lab;
    const int32_t* ord = pk + d.ord;
    const int32_t* slab = ord + d.U;
    for (int32_t i = 0; i < d.U; ++i) {
      PK2_REQUIRE(lab[i] >= 0 && lab[i] < V && lab[i] != blank, "transducer: utterance %d: label %d at %d (%d columns, blank %d)", n,
                  lab[i], i, V, blank);
      PK2_REQUIRE(ord[i] >= 0 && ord[i] < d.U && lab[ord[i]] == slab[i] &&
                      (i == 0 || slab[i - 1] < slab[i] || (slab[i - 1] == slab[i] && ord[i - 1] < ord[i])),
                  "transducer: utterance %d: label positions not sorted by (label, position) at %d", n, i);
    }
    *ws_words += td_layout(d.T, d.U).words;
    *Tmax = std::max(*Tmax, d.T);
    *Umax = std::max(*Umax, d.U);
  }
  return PK2_OK;
}

inline bool td_fits(int64_t rows, int64_t stride, int32_t V) { return stride >= 0 && (rows - 1) * stride + V < (int64_t)1 << 31; }

}  // namespace

extern "C" {

size_t pk2_transducer_workspace_bytes(const int32_t* packed, int32_t num_utts, int32_t num_classes) {
  (void)num_classes;      // the workspace has no term in V: that is the point
  if (!packed || num_utts < 1) return 0;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(packed);
  size_t words = 0;
  for (int32_t n = 0; n < num_utts; ++n)
    if (desc[n].T >= 1 && desc[n].U >= 0 && desc[n].U <= PK2_TRANSDUCER_MAX_LABELS) words += td_layout(desc[n].T, desc[n].U).words;
  return pk2::align_up(words * 4 + 256, 256);
}

int pk2_transducer_loss_and_grad(const int32_t* packed, const int32_t* packed_dev, int64_t packed_words, int32_t num_utts, const float* am,
                                 int64_t am_seq_stride, int64_t am_row_stride, int32_t Tpad, const float* lm, int64_t lm_seq_stride,
                                 int64_t lm_row_stride, int32_t Upad1, int32_t num_classes, int32_t blank, float* grad_am,
                                 int64_t gam_seq_stride, int64_t gam_row_stride, float* grad_lm, int64_t glm_seq_stride,
                                 int64_t glm_row_stride, double* loss, int32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
  PK2_REQUIRE(packed && packed_dev && am && lm && grad_am && grad_lm && loss && status && workspace,
              "pk2_transducer_loss_and_grad: null argument");
  PK2_REQUIRE(num_classes >= 2 && blank >= 0 && blank < num_classes, "transducer: blank %d of %d columns", blank, num_classes);
  PK2_REQUIRE(Tpad >= 1 && Upad1 >= 1 && am_seq_stride >= 0 && lm_seq_stride >= 0 && gam_seq_stride >= 0 && glm_seq_stride >= 0 &&
                  td_fits(Tpad, am_row_stride, num_classes) && td_fits(Upad1, lm_row_stride, num_classes) &&
                  td_fits(Tpad, gam_row_stride, num_classes) && td_fits(Upad1, glm_row_stride, num_classes),
              "transducer: bad strides (an utterance's rows must span fewer than 2^31 floats)");
  size_t ws_words;
  int32_t Tmax, Umax;
  const int rc = td_check(packed, packed_words, num_utts, Tpad, Upad1, num_classes, blank, &ws_words, &Tmax, &Umax);
  if (rc != PK2_OK) return rc;
  const size_t need = pk2::align_up(ws_words * 4 + 256, 256);
  PK2_REQUIRE(workspace_bytes >= need, "transducer: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "transducer: the workspace must be 256-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  const TdTensors p = {am, am_seq_stride, am_row_stride, lm, lm_seq_stride, lm_row_stride, grad_am, gam_seq_stride, gam_row_stride,
                       grad_lm, glm_seq_stride, glm_row_stride, Tpad, Upad1, num_classes, blank};
  const int U1max = Umax + 1, V = num_classes;
  auto tiles = [](int x) { return (x + kTile - 1) / kTile; };
  hipLaunchKernelGGL(td_rows, dim3(std::min(256, (Tmax + U1max + 3) / 4), num_utts), dim3(256), 0, stream, packed_dev, p, ws);
  hipLaunchKernelGGL(td_product<0>, dim3(tiles(U1max), tiles(Tmax), num_utts), dim3(kMmThreads), 0, stream, packed_dev, p, ws, status);
  hipLaunchKernelGGL(td_lattice, dim3(2, num_utts), dim3((U1max + 63) / 64 * 64), 0, stream, packed_dev, ws, loss, status);
  hipLaunchKernelGGL(td_occ, dim3(std::min(1024, (int)(((size_t)Tmax * U1max + 255) / 256)), num_utts), dim3(256), 0, stream, packed_dev,
                     ws, status);
  hipLaunchKernelGGL(td_product<1>, dim3(tiles(V), tiles(Tpad), num_utts), dim3(kMmThreads), 0, stream, packed_dev, p, ws, status);
  hipLaunchKernelGGL(td_product<2>, dim3(tiles(V), tiles(Upad1), num_utts), dim3(kMmThreads), 0, stream, packed_dev, p, ws, status);
  hipLaunchKernelGGL(td_fix, dim3(Tmax + U1max, num_utts), dim3(64), 0, stream, packed_dev, p, ws, status, Tmax);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

int pk2_transducer_greedy(const int32_t* lengths, const int32_t* lengths_dev, int32_t num_utts, const float* am, int64_t seq_stride,
                          int64_t frame_stride, int32_t T, const float* table, int64_t table_stride, int32_t num_classes, int32_t blank,
                          int32_t max_symbols, int32_t* out_tokens, int32_t* out_lens, void* stream_) {
  PK2_REQUIRE(lengths && lengths_dev && am && table && out_tokens && out_lens, "pk2_transducer_greedy: null argument");
  PK2_REQUIRE(num_utts >= 1 && T >= 0 && num_classes >= 2 && blank >= 0 && blank < num_classes && max_symbols >= 1 &&
                  (int64_t)T * max_symbols < (int64_t)1 << 31 && seq_stride >= 0 && frame_stride >= 0 && table_stride >= num_classes,
              "transducer: greedy: %d utterances of %d frames, blank %d of %d columns, %d symbols per frame", num_utts, T, blank, num_classes,
              max_symbols);
  for (int32_t n = 0; n < num_utts; ++n)
    PK2_REQUIRE(lengths[n] >= 0 && lengths[n] <= T, "transducer: greedy: utterance %d has %d frames, the tensor %d", n, lengths[n], T);
  hipLaunchKernelGGL(td_greedy, dim3(num_utts), dim3(64), 0, static_cast<hipStream_t>(stream_), lengths_dev, am, seq_stride, frame_stride,
                     table, table_stride, num_classes, blank, max_symbols, T * max_symbols, out_tokens, out_lens);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

}  // extern "C"
