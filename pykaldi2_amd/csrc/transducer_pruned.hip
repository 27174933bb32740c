// The PRUNED transducer loss on gfx950 (k2's rnnt_loss_pruned and do_rnnt_pruning): the second stage behind
// csrc/transducer.hip.  The first stage's occupancies say which S predictor rows matter at each frame (begin[t]); a
// nonlinear joiner is evaluated on that band only, logits [N][T][S][V], and the loss and its gradient are taken there.
//
//   tr_ranges   pk2_transducer_ranges: one workgroup per utterance.  gamma = occ_x + occ_y from the workspace the first stage
//               left on the stream; per frame (a thread each) the arg-max over the window sums, every window summed on its own
//               in float64 in ascending u; then ONE wave runs the two monotone passes backwards over t as wave scans (a
//               suffix minimum, and a suffix maximum of b[t] - (S-1) t), 64 frames a step with a carry.
//   tp_rows     first pass over the logits: per row (t, s) the maximum and the sum of exponentials in ONE sweep (online
//               rescale), 16-byte loads with a scalar head and tail, the blank and the label column -> px, py, lse [T][S].
//               Rows of V >= PK2_TRANSDUCER_PRUNED_SHORT_ROWS: a wave per row.  Shorter rows: 16 lanes per row, four rows a
//               wave, reduced with __shfl_xor inside the 16.
//   tp_lattice  grid (2, N), ONE wave per chain, no LDS, no barrier: alpha / beta along the anti-diagonals d = t + u.  Lane
//               t mod 64 owns frame t; t + begin[t] increases strictly, so the frames active on a diagonal are a contiguous run
//               of at most S <= 32 and a lane has at most one cell per diagonal.  A cell needs its lane's last value and the
//               neighbour lane's: one rotating __shfl (lane 63 -> lane 0).  float64 log domain.  px / py of a lane's NEXT cell
//               are loaded when the current one is done, at least a diagonal ahead.  Both chains validate begin (status 2)
//               before using it; the alpha chain also scans lse for non-finite rows (status 3), writes loss and status.
//   tp_grad     second pass over the logits, the row split of tp_rows: the head of a row forms occ_x / occ_y in double from
//               alpha, beta, px, py, log p; the sweep writes w (gamma exp(z - lse) - one-hot terms), 16-byte stores aligned on
//               the GRADIENT's row (16-byte loads when the logit row has the same phase, else four scalar loads).  Rows outside
//               the lattice or of an utterance with a status are zeros without a load.
//   tj_fwd / tj_bwd   the banded join h = tanh(enc[t] + pred[begin[t] + s]) and its two gradients, without the gathered
//               copies; d_pred[u] sums the contiguous run of frames whose band holds u (two binary searches), ascending t.
// No float atomics, nothing read back, every launch on the caller's stream.  There is no matrix product anywhere in this file.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "transducer_layout.h"

namespace {

using namespace pk2td;

constexpr int kShortV = PK2_TRANSDUCER_PRUNED_SHORT_ROWS;
constexpr int kShortG = 16;      // lanes per row below kShortV columns

// ------------------------------------------------------------------ ranges
__global__ __launch_bounds__(256) void tr_ranges(const int32_t* __restrict__ pk, const float* __restrict__ ws,
                                                 const int32_t* __restrict__ status, int32_t S, int32_t Tpad, int32_t Upad1,
                                                 int32_t* __restrict__ begin, float* __restrict__ gamma) {
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(pk);
  const TdDesc d = desc[n];
  const int T = d.T, U = d.U, U1 = U + 1;
  const TdLayout l = td_layout(T, U);
  const float* base = ws + td_base(desc, n);
  const float* oy = base + l.oy;
  const float* ox = base + l.ox;
  const bool ok = status[n] == PK2_TRANSDUCER_OK;
  float* g = gamma + (size_t)n * Tpad * Upad1;
  int32_t* bg = begin + (size_t)n * Tpad;
  for (int c = tid; c < Tpad * Upad1; c += 256) {
    const int t = c / Upad1, u = c % Upad1;
    g[c] = (ok && t < T && u < U1) ? ox[(size_t)t * U1 + u] + oy[(size_t)t * U1 + u] : 0.f;
  }
  __syncthreads();
  const int Bmax = max(0, U1 - S);
  for (int t = tid; t < Tpad; t += 256) {
    int arg = 0;
    if (t < T) {
      double best = 0.0;
      for (int s = 0; s <= Bmax; ++s) {
        double win = 0.0;
        for (int u = s; u <= min(s + S - 1, U); ++u) win += (double)g[(size_t)t * Upad1 + u];
        if (s == 0 || win > best) { best = win; arg = s; }
      }
      arg = min(max(arg, max(0, Bmax - (S - 1) * (T - 1 - t))), min(Bmax, (S - 1) * t));
    }
    bg[t] = arg;
  }
  __syncthreads();
  if (tid >= 64) return;
  int cmin = INT_MAX, cmax = INT_MIN;      // the carries from the frames behind
  for (int k = (T - 1) / 64; k >= 0; --k) {
    const int t = k * 64 + lane;
    int v = t < T ? bg[t] : INT_MAX;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_down(v, o, 64);
      if (lane + o < 64) v = min(v, x);
    }
    v = min(v, cmin);
    cmin = __shfl(v, 0, 64);
    int e = t < T ? v - (S - 1) * t : INT_MIN;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_down(e, o, 64);
      if (lane + o < 64) e = max(e, x);
    }
    e = max(e, cmax);
    cmax = __shfl(e, 0, 64);
    if (t < T) bg[t] = e + (S - 1) * t;
  }
}

// ------------------------------------------------------------------ the pruned loss
struct TpArgs {
  const float* z; int64_t zn, zt, zs;      // logits: row (n, t, s) at [n zn + t zt + s zs], unit column stride
  float* g;                                // gradient, dense [N][Tpad][S][V]
  const int32_t* begin;                    // dense [N][Tpad]
  int32_t Tpad, S, V, blank;
};
struct TpWs {      // all [N][Tpad][S] but lp [N]
  float *px, *py, *lse;
  double *al, *be, *lp;
};
inline TpWs tp_carve(void* workspace, size_t N, size_t Tpad, size_t S, size_t* bytes) {
  pk2::Carver c(workspace);
  const size_t cells = N * Tpad * S;
  TpWs w;
  w.px = c.take<float>(cells);
  w.py = c.take<float>(cells);
  w.lse = c.take<float>(cells);
  w.al = c.take<double>(cells);
  w.be = c.take<double>(cells);
  w.lp = c.take<double>(N);
  *bytes = c.bytes();
  return w;
}

template <int G>
__device__ __forceinline__ float tp_group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float tp_group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One more value into (m, s) = (maximum so far, sum of exp(. - m)).  +inf and NaN end as a NaN sum, a row of -inf as m = -inf.
__device__ __forceinline__ void tp_push(float& m, float& s, float x) {
  if (x > m) { s = m > -INFINITY ? s * __expf(m - x) : 0.f; m = x; }
  if (m > -INFINITY) s += __expf(x - m);
}
__device__ __forceinline__ void tp_push4(float& m, float& s, const float4 q) {
  const float m4 = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  if (m4 > m) { s = m > -INFINITY ? s * __expf(m - m4) : 0.f; m = m4; }
  if (m > -INFINITY) s += (__expf(q.x - m) + __expf(q.y - m)) + (__expf(q.z - m) + __expf(q.w - m));
}

// grid (blocks, N); G lanes per row, rows (t, s) of the utterance's own frames only.
template <int G>
__global__ __launch_bounds__(256) void tp_rows(const int32_t* __restrict__ pk, TpArgs p, TpWs w) {
  const int n = blockIdx.y, gl = threadIdx.x % G;
  const int grp = blockIdx.x * (256 / G) + threadIdx.x / G, ngrp = gridDim.x * (256 / G);
  const TdDesc d = reinterpret_cast<const TdDesc*>(pk)[n];
  const int T = d.T, U = d.U, S = p.S, V = p.V;
  const int32_t* lab = pk + d.lab;
  const int32_t* bg = p.begin + (size_t)n * p.Tpad;
  for (int r = grp; r < T * S; r += ngrp) {
    const int t = r / S, s = r % S;
    const size_t cell = ((size_t)n * p.Tpad + t) * S + s;
    const int64_t u = (int64_t)bg[t] + s;
    if (u < 0 || u > U) {      // not a cell of the lattice (or a band that tp_lattice will refuse): nothing is indexed with u
      if (gl == 0) { w.px[cell] = -INFINITY; w.py[cell] = -INFINITY; w.lse[cell] = 0.f; }
      continue;
    }
    const float* row = p.z + n * p.zn + t * p.zt + s * p.zs;
    // the row as [head scalars][16-byte aligned float4s][tail scalars]; the scalars are at most 6, one lane each
    const int head = min(V, (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) >> 2));
    const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
    float m = -INFINITY, sum = 0.f;
    for (int v = gl; v < nvec; v += G) tp_push4(m, sum, *reinterpret_cast<const float4*>(row + head + 4 * v));
    if (gl < head + V - tail0) tp_push(m, sum, row[gl < head ? gl : tail0 + gl - head]);
    const float M = tp_group_max<G>(m);
    sum = tp_group_sum<G>(m > -INFINITY ? sum * __expf(m - M) : 0.f);
    if (gl == 0) {
      const double lse = (double)M + log((double)sum);
      w.lse[cell] = (float)lse;
      w.py[cell] = (float)((double)row[p.blank] - lse);
      w.px[cell] = u < U ? (float)((double)row[lab[u]] - lse) : -INFINITY;
    }
  }
}

// begin[0] = 0, steps in [0, S-1], begin[T-1] + S - 1 >= U, nothing negative: by the whole wave.
__device__ __forceinline__ bool tp_band_ok(const int32_t* bg, int T, int U, int S, int lane) {
  bool bad = false;
  for (int t = lane; t < T; t += 64) {
    const int64_t b = bg[t], step = t ? b - (int64_t)bg[t - 1] : 0;
    bad = bad || b < 0 || (t == 0 && b != 0) || step < 0 || step > S - 1 || (t == T - 1 && b + S - 1 < U);
  }
  return !__any(bad);
}

// grid (2, N), one wave.  blockIdx.x = 0: alpha, loss, status; 1: beta.
__global__ __launch_bounds__(64) void tp_lattice(const int32_t* __restrict__ pk, TpArgs p, TpWs w, double* __restrict__ loss,
                                                 int32_t* __restrict__ status) {
  const int n = blockIdx.y, lane = threadIdx.x;
  const bool fwd = blockIdx.x == 0;
  const TdDesc d = reinterpret_cast<const TdDesc*>(pk)[n];
  const int T = d.T, U = d.U, S = p.S, D = T + U;
  const int32_t* bg = p.begin + (size_t)n * p.Tpad;
  const size_t cell0 = (size_t)n * p.Tpad * S;
  const float* px = w.px + cell0;
  const float* py = w.py + cell0;
  const double NEG = -INFINITY;
  if (!tp_band_ok(bg, T, U, S, lane)) {
    if (fwd && lane == 0) { loss[n] = 0.0; status[n] = PK2_TRANSDUCER_RANGES; w.lp[n] = 0.0; }
    return;
  }
  // the lane's cells in the order of the diagonals: (t, s) its pending cell, diag its diagonal, xn / yn its px / py
  int t, s = 0, bt = 0, hi = -1, diag;
  float xn = 0.f, yn = 0.f;
  double pub = NEG;      // what the neighbour lane reads on the next diagonal, and the frame it belongs to
  int pubt = -2;
  if (fwd) {
    bool bad = false;
    for (int c = lane; c < T * S; c += 64)
      if (bg[c / S] + c % S <= U) bad = bad || !(fabsf(w.lse[cell0 + c]) < INFINITY);
    const bool numeric = !__any(bad);
    double* al = w.al + cell0;
    auto enter = [&]() {
      while (t < T) {
        bt = bg[t];
        hi = min(bt + S - 1, U);
        if (hi >= bt) break;
        t += 64;
      }
      s = 0;
      diag = INT_MAX;
      if (t < T) { diag = t + bt; xn = px[(size_t)t * S]; yn = py[(size_t)t * S]; }
    };
    t = lane;
    enter();
    double right = NEG, lp = NEG;      // right: alpha + px of the lane's last cell
    for (int dg = 0; dg < D; ++dg) {
      const double nb = __shfl(pub, (lane + 63) & 63, 64);
      const int nbt = __shfl(pubt, (lane + 63) & 63, 64);
      pub = NEG;
      pubt = -2;
      if (diag == dg) {
        const int u = bt + s;
        const double a = (t == 0 && u == 0) ? 0.0 : pk2::log_add(nbt == t - 1 ? nb : NEG, right);
        al[(size_t)t * S + s] = a;
        pub = a + (double)yn;
        pubt = t;
        right = a + (double)xn;      // (px is -inf at u = U)
        if (t == T - 1 && u == U) lp = pub;
        if (u < hi) {
          ++s; ++diag;
          xn = px[(size_t)t * S + s]; yn = py[(size_t)t * S + s];
        } else {
          t += 64;
          right = NEG;
          enter();
        }
      }
    }
    lp = __shfl(lp, (T - 1) & 63, 64);
    if (lane == 0) {
      const bool ok = numeric && lp == lp && lp > -INFINITY && lp < INFINITY;
      w.lp[n] = lp;
      loss[n] = ok ? -lp : 0.0;
      status[n] = ok ? PK2_TRANSDUCER_OK : PK2_TRANSDUCER_NUMERIC;
    }
  } else {
    double* be = w.be + cell0;
    auto enter = [&]() {
      while (t >= 0) {
        bt = bg[t];
        hi = min(bt + S - 1, U);
        if (hi >= bt) break;
        t -= 64;
      }
      diag = INT_MIN;
      if (t >= 0) { s = hi - bt; diag = t + hi; xn = px[(size_t)t * S + s]; yn = py[(size_t)t * S + s]; }
    };
    t = lane < T ? lane + ((T - 1 - lane) / 64) * 64 : -1;
    enter();
    double own = NEG;      // beta of the lane's last cell, (t, u + 1)
    for (int dg = D - 1; dg >= 0; --dg) {
      const double nb = __shfl(pub, (lane + 1) & 63, 64);
      const int nbt = __shfl(pubt, (lane + 1) & 63, 64);
      pub = NEG;
      pubt = -2;
      if (diag == dg) {
        const int u = bt + s;
        const double below = t == T - 1 ? (u == U ? 0.0 : NEG) : (nbt == t + 1 ? nb : NEG);
        const double b = pk2::log_add((double)yn + below, (double)xn + own);
        be[(size_t)t * S + s] = b;
        pub = b;
        pubt = t;
        own = b;
        if (s > 0) {
          --s; --diag;
          xn = px[(size_t)t * S + s]; yn = py[(size_t)t * S + s];
        } else {
          t -= 64;
          own = NEG;
          enter();
        }
      }
    }
  }
}

// grid (blocks, N); G lanes per row, ALL rows (t, s) of the tensor.
template <int G>
__global__ __launch_bounds__(256) void tp_grad(const int32_t* __restrict__ pk, TpArgs p, TpWs w, const int32_t* __restrict__ status) {
  const int n = blockIdx.y, gl = threadIdx.x % G;
  const int grp = blockIdx.x * (256 / G) + threadIdx.x / G, ngrp = gridDim.x * (256 / G);
  const TdDesc d = reinterpret_cast<const TdDesc*>(pk)[n];
  const int T = d.T, U = d.U, S = p.S, V = p.V;
  const int32_t* lab = pk + d.lab;
  const int32_t* bg = p.begin + (size_t)n * p.Tpad;
  const bool ok = status[n] == PK2_TRANSDUCER_OK;      // then the band is valid
  const double lp = w.lp[n];
  const size_t cell0 = (size_t)n * p.Tpad * S;
  for (int r = grp; r < p.Tpad * S; r += ngrp) {
    const int t = r / S, s = r % S;
    float* grow = p.g + (cell0 + r) * V;
    const int head = min(V, (int)(((16 - (reinterpret_cast<uintptr_t>(grow) & 15)) & 15) >> 2));
    const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
    const int u = ok && t < T ? bg[t] + s : -1;
    if (u < 0 || u > U) {
      for (int v = gl; v < nvec; v += G) *reinterpret_cast<float4*>(grow + head + 4 * v) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gl < head + V - tail0) grow[gl < head ? gl : tail0 + gl - head] = 0.f;
      continue;
    }
    const size_t cell = cell0 + r;
    const double a = w.al[cell] - lp;
    double by = u == U ? 0.0 : -INFINITY;      // beta[t + 1, u]
    if (t + 1 < T) {
      const int s2 = u - bg[t + 1];
      by = s2 >= 0 && s2 < S ? w.be[cell0 + (size_t)(t + 1) * S + s2] : -INFINITY;
    }
    const double oy = exp(a + (double)w.py[cell] + by);
    const double ox = u < U && s + 1 < S ? exp(a + (double)w.px[cell] + w.be[cell + 1]) : 0.0;
    const float gam = (float)(ox + oy), foy = (float)oy, fox = (float)ox, wn = d.w, lse = w.lse[cell];
    const int blank = p.blank, lb = u < U ? lab[u] : -1;
    const float* row = p.z + n * p.zn + t * p.zt + s * p.zs;
    auto val = [&](int v, float z) { return wn * (gam * __expf(z - lse) - (v == blank ? foy : 0.f) - (v == lb ? fox : 0.f)); };
    const bool same = ((reinterpret_cast<uintptr_t>(row) ^ reinterpret_cast<uintptr_t>(grow)) & 15) == 0;
    for (int v = gl; v < nvec; v += G) {
      const int c = head + 4 * v;
      float4 q;
      if (same) q = *reinterpret_cast<const float4*>(row + c);
      else q = make_float4(row[c], row[c + 1], row[c + 2], row[c + 3]);
      *reinterpret_cast<float4*>(grow + c) = make_float4(val(c, q.x), val(c + 1, q.y), val(c + 2, q.z), val(c + 3, q.w));
    }
    if (gl < head + V - tail0) {
      const int c = gl < head ? gl : tail0 + gl - head;
      grow[c] = val(c, row[c]);
    }
  }
}

// ------------------------------------------------------------------ the banded join
struct TjArgs {
  const int32_t* lens;                     // device [N][2]: frames T_n, labels U_n
  const int32_t* begin;                    // dense [N][Tpad]
  int32_t Tpad, Upad1, S, J, use_tanh;
};

// grid (blocks, N): an element (a float, or with VEC four) per thread, rows (t, s) of h [N][Tpad][S][J].
template <bool VEC>
__global__ __launch_bounds__(256) void tj_fwd(TjArgs p, const float* __restrict__ enc, int64_t en, int64_t et,
                                              const float* __restrict__ pred, int64_t pn, int64_t pu, float* __restrict__ h) {
  const int n = blockIdx.y, T = p.lens[2 * n], U = p.lens[2 * n + 1], S = p.S;
  const int Jv = VEC ? p.J / 4 : p.J;
  const int32_t* bg = p.begin + (size_t)n * p.Tpad;
  float* hn = h + (size_t)n * p.Tpad * S * p.J;
  const int64_t total = (int64_t)p.Tpad * S * Jv;
  for (int64_t e = blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / Jv), j = (int)(e % Jv), t = r / S, s = r % S;
    const int64_t u = t < T ? (int64_t)bg[t] + s : -1;
    const bool live = u >= 0 && u <= U;
    const float* a = enc + n * en + t * et;
    const float* b = pred + n * pn + u * pu;
    if (VEC) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        const float4 x = reinterpret_cast<const float4*>(a)[j], y = reinterpret_cast<const float4*>(b)[j];
        o = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
        if (p.use_tanh) o = make_float4(tanhf(o.x), tanhf(o.y), tanhf(o.z), tanhf(o.w));
      }
      reinterpret_cast<float4*>(hn)[e] = o;
    } else {
      float o = 0.f;
      if (live) {
        o = a[j] + b[j];
        if (p.use_tanh) o = tanhf(o);
      }
      hn[e] = o;
    }
  }
}

// grid (Tpad + Upad1, N): workgroup x < Tpad owns row x of d_enc, the others row x - Tpad of d_pred.
template <bool VEC>
__global__ __launch_bounds__(256) void tj_bwd(TjArgs p, const float* __restrict__ dh, const float* __restrict__ h,
                                              float* __restrict__ d_enc, float* __restrict__ d_pred) {
  const int n = blockIdx.y, T = p.lens[2 * n], U = p.lens[2 * n + 1], S = p.S, J = p.J;
  const int Jv = VEC ? J / 4 : J;
  const int32_t* bg = p.begin + (size_t)n * p.Tpad;
  const size_t base = (size_t)n * p.Tpad * S * J;
  const bool is_enc = (int)blockIdx.x < p.Tpad;
  const int x = is_enc ? blockIdx.x : blockIdx.x - p.Tpad;
  float* out = is_enc ? d_enc + ((size_t)n * p.Tpad + x) * J : d_pred + ((size_t)n * p.Upad1 + x) * J;
  int lo = 0, hi = 0;      // the rows (t, s) to add: is_enc: s in [lo, hi) of frame x; else frames [lo, hi) at s = x - begin[t]
  if (is_enc) {
    if (x < T) hi = S;
  } else if (x <= U) {
    int a = 0, b = T;      // first t with begin[t] + S - 1 >= x
    while (a < b) {
      const int m = (a + b) >> 1;
      if ((int64_t)bg[m] + S - 1 >= x) b = m; else a = m + 1;
    }
    lo = a;
    b = T;                 // first t with begin[t] > x
    while (a < b) {
      const int m = (a + b) >> 1;
      if (bg[m] > x) b = m; else a = m + 1;
    }
    hi = a;
  }
  for (int j = threadIdx.x; j < Jv; j += 256) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = lo; k < hi; ++k) {
      const int t = is_enc ? x : k;
      const int64_t s = is_enc ? k : (int64_t)x - bg[t], u = is_enc ? (int64_t)bg[t] + k : x;
      if (s < 0 || s >= S || u < 0 || u > U) continue;
      const size_t row = base + ((size_t)t * S + s) * J;
      if (VEC) {
        const float4 g = reinterpret_cast<const float4*>(dh + row)[j];
        float4 f = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p.use_tanh) {
          const float4 y = reinterpret_cast<const float4*>(h + row)[j];
          f = make_float4(1.f - y.x * y.x, 1.f - y.y * y.y, 1.f - y.z * y.z, 1.f - y.w * y.w);
        }
        acc.x += g.x * f.x; acc.y += g.y * f.y; acc.z += g.z * f.z; acc.w += g.w * f.w;
      } else {
        const float y = p.use_tanh ? h[row + j] : 0.f;
        acc.x += dh[row + j] * (1.f - y * y);
      }
    }
    if (VEC) reinterpret_cast<float4*>(out)[j] = acc;
    else out[j] = acc.x;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int tj_check(const int32_t* lens, int32_t N, int32_t Tpad, int32_t Upad1, int32_t S, int32_t J) {
  PK2_REQUIRE(N >= 1 && Tpad >= 1 && Upad1 >= 1 && J >= 1 && S >= 2 && S <= PK2_TRANSDUCER_MAX_PRUNE_RANGE &&
                  (int64_t)Tpad * S * J < (int64_t)1 << 31,
              "transducer join: %d utterances, %d frames, %d predictor rows, band %d, %d columns", N, Tpad, Upad1, S, J);
  for (int32_t n = 0; n < N; ++n)
    PK2_REQUIRE(lens[2 * n] >= 0 && lens[2 * n] <= Tpad && lens[2 * n + 1] >= 0 && lens[2 * n + 1] < Upad1,
                "transducer join: utterance %d has %d frames and %d labels, the tensors %d frames and %d rows", n, lens[2 * n],
                lens[2 * n + 1], Tpad, Upad1);
  return PK2_OK;
}

}  // namespace

extern "C" {

int pk2_transducer_ranges(const int32_t* packed, const int32_t* packed_dev, int64_t packed_words, int32_t num_utts, int32_t prune_range,
                          int32_t Tpad, int32_t Upad1, const int32_t* status, const void* workspace, size_t workspace_bytes,
                          int32_t* begin, float* gamma, void* stream) {
  PK2_REQUIRE(packed && packed_dev && status && workspace && begin && gamma, "pk2_transducer_ranges: null argument");
  const int32_t S = prune_range;
  PK2_REQUIRE(S >= 2 && S <= PK2_TRANSDUCER_MAX_PRUNE_RANGE, "transducer: prune range %d outside [2, %d]", S, PK2_TRANSDUCER_MAX_PRUNE_RANGE);
  PK2_REQUIRE(num_utts >= 1 && packed_words >= (int64_t)num_utts * 8 && Tpad >= 1 && Upad1 >= 1 && (int64_t)Tpad * Upad1 < (int64_t)1 << 31,
              "transducer: ranges for %d utterances, %d frames, %d predictor rows", num_utts, Tpad, Upad1);
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(packed);
  size_t words = 0;
  for (int32_t n = 0; n < num_utts; ++n) {
    const TdDesc& d = desc[n];
    PK2_REQUIRE(d.T >= 1 && d.T <= Tpad && d.U >= 0 && d.U < Upad1 && d.U <= PK2_TRANSDUCER_MAX_LABELS,
                "transducer: utterance %d has %d frames and %d labels, the outputs %d and %d rows", n, d.T, d.U, Tpad, Upad1);
    PK2_REQUIRE(std::max(0, d.U + 1 - S) <= (int64_t)(S - 1) * (d.T - 1),
                "transducer: utterance %d: %d labels cannot be covered by a band of %d over %d frames", n, d.U, S, d.T);
    words += td_layout(d.T, d.U).words;
  }
  PK2_REQUIRE(workspace_bytes >= pk2::align_up(words * 4 + 256, 256), "transducer: ranges: not the first stage's workspace (%zu bytes)",
              workspace_bytes);
  hipLaunchKernelGGL(tr_ranges, dim3(num_utts), dim3(256), 0, static_cast<hipStream_t>(stream), packed_dev,
                     static_cast<const float*>(workspace), status, S, Tpad, Upad1, begin, gamma);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

size_t pk2_transducer_pruned_workspace_bytes(int32_t num_utts, int32_t Tpad, int32_t prune_range, int32_t num_classes) {
  (void)num_classes;      // no term in V
  if (num_utts < 1 || Tpad < 1 || prune_range < 1) return 0;
  size_t bytes;
  tp_carve(nullptr, num_utts, Tpad, prune_range, &bytes);
  return bytes;
}

int pk2_transducer_pruned_loss_and_grad(const int32_t* packed, const int32_t* packed_dev, int64_t packed_words, int32_t num_utts,
                                        const float* logits, int64_t seq_stride, int64_t frame_stride, int64_t band_stride, int32_t Tpad,
                                        int32_t prune_range, int32_t num_classes, int32_t blank, const int32_t* begin, float* grad,
                                        double* loss, int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
  PK2_REQUIRE(packed && packed_dev && logits && begin && grad && loss && status && workspace,
              "pk2_transducer_pruned_loss_and_grad: null argument");
  const int32_t S = prune_range, V = num_classes, N = num_utts;
  PK2_REQUIRE(V >= 2 && blank >= 0 && blank < V, "transducer: blank %d of %d columns", blank, V);
  PK2_REQUIRE(S >= 2 && S <= PK2_TRANSDUCER_MAX_PRUNE_RANGE, "transducer: prune range %d outside [2, %d]", S, PK2_TRANSDUCER_MAX_PRUNE_RANGE);
  PK2_REQUIRE(N >= 1 && packed_words >= (int64_t)N * 8 && Tpad >= 1 && (int64_t)Tpad * S < (int64_t)1 << 31 && seq_stride >= 0 &&
                  frame_stride >= 0 && band_stride >= 0,
              "transducer: pruned loss for %d utterances of %d frames, band %d: bad sizes or strides", N, Tpad, S);
  const TdDesc* desc = reinterpret_cast<const TdDesc*>(packed);
  for (int32_t n = 0; n < N; ++n) {
    const TdDesc& d = desc[n];
    PK2_REQUIRE(d.T >= 1 && d.T <= Tpad, "transducer: utterance %d has %d frames, the tensor %d", n, d.T, Tpad);
    if (d.U < 0 || d.U > PK2_TRANSDUCER_MAX_LABELS) {
      pk2::set_error("transducer: utterance %d has %d labels (limit %d)", n, d.U, PK2_TRANSDUCER_MAX_LABELS);
      return PK2_ERR_LIMIT;
    }
    PK2_REQUIRE(d.lab >= N * 8 && (int64_t)d.lab + d.U <= packed_words, "transducer: utterance %d: labels outside the descriptor", n);
    for (int32_t i = 0; i < d.U; ++i)
      PK2_REQUIRE(packed[d.lab + i] >= 0 && packed[d.lab + i] < V && packed[d.lab + i] != blank,
                  "transducer: utterance %d: label %d at %d (%d columns, blank %d)", n, packed[d.lab + i], i, V, blank);
  }
  size_t need;
  const TpWs w = tp_carve(workspace, N, Tpad, S, &need);
  PK2_REQUIRE(workspace_bytes >= need, "transducer: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "transducer: the workspace must be 256-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const TpArgs p = {logits, seq_stride, frame_stride, band_stride, grad, begin, Tpad, S, V, blank};
  const int rows = Tpad * S;
  if (V >= kShortV) {
    const dim3 grid(std::min(4096, (rows + 3) / 4), N);
    hipLaunchKernelGGL(tp_rows<64>, grid, dim3(256), 0, stream, packed_dev, p, w);
    hipLaunchKernelGGL(tp_lattice, dim3(2, N), dim3(64), 0, stream, packed_dev, p, w, loss, status);
    hipLaunchKernelGGL(tp_grad<64>, grid, dim3(256), 0, stream, packed_dev, p, w, status);
  } else {
    const dim3 grid(std::min(4096, (rows + 256 / kShortG - 1) / (256 / kShortG)), N);
    hipLaunchKernelGGL(tp_rows<kShortG>, grid, dim3(256), 0, stream, packed_dev, p, w);
    hipLaunchKernelGGL(tp_lattice, dim3(2, N), dim3(64), 0, stream, packed_dev, p, w, loss, status);
    hipLaunchKernelGGL(tp_grad<kShortG>, grid, dim3(256), 0, stream, packed_dev, p, w, status);
  }
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

int pk2_transducer_join(const int32_t* lens, const int32_t* lens_dev, int32_t num_utts, const float* enc, int64_t enc_seq_stride,
                        int64_t enc_row_stride, const float* pred, int64_t pred_seq_stride, int64_t pred_row_stride, const int32_t* begin,
                        int32_t Tpad, int32_t Upad1, int32_t prune_range, int32_t dim, int32_t use_tanh, float* h, void* stream) {
  PK2_REQUIRE(lens && lens_dev && enc && pred && begin && h, "pk2_transducer_join: null argument");
  PK2_REQUIRE(enc_seq_stride >= 0 && enc_row_stride >= 0 && pred_seq_stride >= 0 && pred_row_stride >= 0, "transducer join: negative stride");
  const int rc = tj_check(lens, num_utts, Tpad, Upad1, prune_range, dim);
  if (rc != PK2_OK) return rc;
  const TjArgs p = {lens_dev, begin, Tpad, Upad1, prune_range, dim, use_tanh};
  const bool vec = dim % 4 == 0 && al16(enc) && al16(pred) && al16(h) && enc_seq_stride % 4 == 0 && enc_row_stride % 4 == 0 &&
                   pred_seq_stride % 4 == 0 && pred_row_stride % 4 == 0;
  const int64_t total = (int64_t)Tpad * prune_range * (vec ? dim / 4 : dim);
  const dim3 grid((unsigned)std::min<int64_t>(8192, (total + 255) / 256), num_utts);
  if (vec)
    hipLaunchKernelGGL(tj_fwd<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p, enc, enc_seq_stride, enc_row_stride, pred,
                       pred_seq_stride, pred_row_stride, h);
  else
    hipLaunchKernelGGL(tj_fwd<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p, enc, enc_seq_stride, enc_row_stride, pred,
                       pred_seq_stride, pred_row_stride, h);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

int pk2_transducer_join_backward(const int32_t* lens, const int32_t* lens_dev, int32_t num_utts, const float* dh, const float* h,
                                 const int32_t* begin, int32_t Tpad, int32_t Upad1, int32_t prune_range, int32_t dim, int32_t use_tanh,
                                 float* d_enc, float* d_pred, void* stream) {
  PK2_REQUIRE(lens && lens_dev && dh && h && begin && d_enc && d_pred, "pk2_transducer_join_backward: null argument");
  const int rc = tj_check(lens, num_utts, Tpad, Upad1, prune_range, dim);
  if (rc != PK2_OK) return rc;
  const TjArgs p = {lens_dev, begin, Tpad, Upad1, prune_range, dim, use_tanh};
  const bool vec = dim % 4 == 0 && al16(dh) && al16(h) && al16(d_enc) && al16(d_pred);
  const dim3 grid(Tpad + Upad1, num_utts);
  if (vec) hipLaunchKernelGGL(tj_bwd<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p, dh, h, d_enc, d_pred);
  else hipLaunchKernelGGL(tj_bwd<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p, dh, h, d_enc, d_pred);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

}  // extern "C"
