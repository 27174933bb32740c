// Sampling-rate conversion of a ragged minibatch in one launch: Kaldi's LinearResample (polyphase windowed sinc), the
// arithmetic of speed perturbation, with the volume gain folded in (include/pk2hip.h).
//
//   pk2_resample_plan_*   host object: first[] / taps[] per output phase, float32 weights (computed in double)
//   pk2_resample_batch    every job of a minibatch (own plan, own length, own gain) in one launch
//
// Output k = u ou + p of a job reads x[start(k) .. start(k) + taps[p]), start(k) = first[p] + u iu = ceil((k / fo - ww) fi):
// start() and the last index read are non-decreasing in k (checked when the plan is made), so the outputs [k0, k1) of a tile
// read the one span [start(k0), last(k1 - 1)].  A workgroup stages that span in LDS -- zeros outside [0, n_in), the only
// place that looks at the ends of the input -- then every thread forms outputs k0 + tid, k0 + tid + 256, ...: neighbouring
// lanes read neighbouring LDS words and write neighbouring output words.  The weights are stored tap-major (w[j][p]) so that
// the lanes of a wave, which hold consecutive phases, read consecutive words from LDS or from memory.
#include <math.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "common.h"

namespace pk2 {

constexpr int kRsThreads = 256;
constexpr int kRsTileMax = 1024;     // outputs per workgroup, a multiple of kRsThreads
constexpr int kRsSpanMax = 6144;     // staged input samples (24 KB)
constexpr int kRsWLds = 4096;        // weight table staged in LDS when ou * max_taps fits (16 KB) ...
constexpr int kRsPhaseLds = 512;     // ... and ou does (first / taps, 4 KB)

struct RsJobDev {
  const int2* ft;      // (ou) {first, taps}
  const float* w;      // (max_taps, ou) tap-major
  const float* in;
  float* out;
  int64_t n_in, n_out;
  int32_t iu, ou, max_taps, tile;
  float gain;
  int32_t tile_begin;  // first workgroup of the job
  int32_t w_lds, pad_;
};
struct RsJobs {
  RsJobDev j[PK2_RESAMPLE_MAX_JOBS];
  int32_t njobs;
};

template <bool kLds>
__device__ __forceinline__ void resample_tile(const RsJobDev& jb, int64_t k0, float* s_x, float* s_w, int2* s_ft) {
  const int tid = threadIdx.x, ou = jb.ou, iu = jb.iu;
  const int nk = (int)min((int64_t)jb.tile, jb.n_out - k0);
  const int2* __restrict__ ft = jb.ft;
  const float* __restrict__ w = jb.w;
  const float* __restrict__ in = jb.in;
  const int64_t u0 = k0 / ou;
  const int p0 = (int)(k0 - u0 * ou);
  const int ql = p0 + nk - 1, ul = ql / ou, pl = ql - ul * ou;      // the tile's last output, relative to u0
  const int2 f0 = ft[p0], fl = ft[pl];
  const int64_t span0 = (int64_t)f0.x + u0 * iu;
  const int span = min((int)((int64_t)ul * iu + fl.x + fl.y - f0.x), kRsSpanMax);     // (the plan's tile keeps it below)
  const int64_t n_in = jb.n_in;
  for (int i = tid; i < span; i += kRsThreads) {
    const int64_t g = span0 + i;
    s_x[i] = (g >= 0 && g < n_in) ? in[g] : 0.f;
  }
  if (kLds) {
    const int nw = ou * jb.max_taps;
    for (int i = tid; i < nw; i += kRsThreads) s_w[i] = w[i];
    for (int i = tid; i < ou; i += kRsThreads) s_ft[i] = ft[i];
  }
  __syncthreads();
  const float gain = jb.gain;
  float* __restrict__ out = jb.out + k0;
  for (int d = tid; d < nk; d += kRsThreads) {
    const int q = p0 + d, du = q / ou, p = q - du * ou;
    const int2 f = kLds ? s_ft[p] : ft[p];
    const int rel = (int)((int64_t)du * iu + f.x - f0.x);
    const int nt = min(f.y, span - rel);
    float acc = 0.f;
    if (kLds) {
      for (int j = 0; j < nt; ++j) acc = fmaf(s_w[j * ou + p], s_x[rel + j], acc);
    } else {
      for (int j = 0; j < nt; ++j) acc = fmaf(w[(int64_t)j * ou + p], s_x[rel + j], acc);
    }
    out[d] = acc * gain;
  }
}

// grid: the tiles of all jobs, job after job (tile_begin[]).
__global__ void __launch_bounds__(kRsThreads) resample_batch_kernel(const RsJobs jobs) {
  __shared__ float s_x[kRsSpanMax];
  __shared__ float s_w[kRsWLds];
  __shared__ int2 s_ft[kRsPhaseLds];
  const int b = blockIdx.x;
  int ji = 0;
  while (ji + 1 < jobs.njobs && jobs.j[ji + 1].tile_begin <= b) ++ji;       // uniform over the workgroup
  const RsJobDev& jb = jobs.j[ji];
  const int64_t k0 = (int64_t)(b - jb.tile_begin) * jb.tile;
  if (k0 >= jb.n_out) return;
  if (jb.w_lds) resample_tile<true>(jb, k0, s_x, s_w, s_ft);
  else resample_tile<false>(jb, k0, s_x, s_w, s_ft);
}

}  // namespace pk2

using namespace pk2;

struct pk2_resample_plan {
  int32_t rate_in, rate_out, iu, ou, max_taps, tile;
  std::vector<int32_t> first, taps;
  std::vector<float> weights;        // (ou, max_taps) phase-major: what pk2_resample_plan_export hands out
  std::vector<int2> ft_dev_layout;   // (ou)
  std::vector<float> w_dev_layout;   // (max_taps, ou)
  std::mutex mu;
  void* dev_block[PerDevice<int>::kMax];   // per device: {ft, w} in one allocation, made by the first launch there
};

static int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

// The longest input span a tile of `tile` outputs reads, over every phase the tile can start at.
static int64_t rs_max_span(const pk2_resample_plan& P, int tile) {
  int64_t worst = 0;
  for (int p0 = 0; p0 < P.ou; ++p0) {
    const int64_t ql = (int64_t)p0 + tile - 1, ul = ql / P.ou, pl = ql - ul * P.ou;
    worst = std::max(worst, ul * P.iu + P.first[pl] + P.taps[pl] - P.first[p0]);
  }
  return worst;
}

extern "C" int pk2_resample_plan_create(int32_t rate_in, int32_t rate_out, double cutoff_hz, int32_t num_zeros,
                                        pk2_resample_plan** plan_out) {
  PK2_REQUIRE(plan_out, "resample_plan_create: null pointer");
  *plan_out = nullptr;
  PK2_REQUIRE(rate_in > 0 && rate_out > 0, "resample_plan_create: rates must be positive (got %d -> %d)", rate_in, rate_out);
  PK2_REQUIRE(num_zeros >= 1, "resample_plan_create: num_zeros must be at least 1 (got %d)", num_zeros);
  const double half_min = 0.5 * std::min(rate_in, rate_out);
  PK2_REQUIRE(cutoff_hz >= 0.0 && cutoff_hz <= half_min && cutoff_hz == cutoff_hz,
              "resample_plan_create: cutoff %g Hz outside (0, %g] (0 selects the default)", cutoff_hz, half_min);
  const double cutoff = cutoff_hz > 0.0 ? cutoff_hz : 0.99 * half_min;
  const int64_t g = rs_gcd(rate_in, rate_out);
  pk2_resample_plan* P = new pk2_resample_plan();
  P->rate_in = rate_in; P->rate_out = rate_out;
  P->iu = (int32_t)(rate_in / g); P->ou = (int32_t)(rate_out / g);
  memset(P->dev_block, 0, sizeof(P->dev_block));
  const int ou = P->ou;
  P->first.resize(ou); P->taps.resize(ou);
  std::vector<std::vector<float>> rows(ou);
  int max_taps = 0;
  if (rate_in == rate_out) {      // a copy: no filter
    P->first[0] = 0; P->taps[0] = 1; rows[0] = {1.0f};
    max_taps = 1;
  } else {
    const double fi = rate_in, fo = rate_out, ww = num_zeros / (2.0 * cutoff), pi = 3.14159265358979323846;
    for (int p = 0; p < ou; ++p) {
      const double t = p / fo;
      const int64_t lo = (int64_t)ceil((t - ww) * fi), hi = (int64_t)floor((t + ww) * fi);
      const int64_t n = hi - lo + 1;
      if (n < 1 || n > PK2_RESAMPLE_MAX_TAPS) {
        delete P;
        set_error("resample_plan_create: %lld taps at phase %d (1 .. %d supported)", (long long)n, p, PK2_RESAMPLE_MAX_TAPS);
        return PK2_ERR_LIMIT;
      }
      P->first[p] = (int32_t)lo; P->taps[p] = (int32_t)n;
      rows[p].resize(n);
      for (int64_t j = 0; j < n; ++j) {
        const double dt = (lo + j) / fi - t;
        const double h = fabs(dt) < ww ? 0.5 * (1.0 + cos(2.0 * pi * cutoff / num_zeros * dt)) : 0.0;
        const double f = dt != 0.0 ? sin(2.0 * pi * cutoff * dt) / (pi * dt) : 2.0 * cutoff;
        rows[p][j] = (float)(f * h / fi);
      }
      max_taps = std::max(max_taps, (int)n);
    }
  }
  P->max_taps = max_taps;
  // what the kernel's single staged span rests on: the first and the last index read do not decrease from one output to the next
  for (int p = 0; p < ou; ++p) {
    const int q = (p + 1) % ou;
    const int64_t step = q == 0 ? P->iu : 0;
    const int64_t s0 = P->first[p], s1 = P->first[q] + step;
    if (s1 < s0 || s1 + P->taps[q] < s0 + P->taps[p]) {
      delete P;
      set_error("resample_plan_create: the taps of phase %d and its successor are not ordered", p);
      return PK2_ERR_INVALID;
    }
  }
  P->tile = 0;
  for (int tile = kRsTileMax; tile >= kRsThreads; tile -= kRsThreads)
    if (rs_max_span(*P, tile) <= kRsSpanMax) { P->tile = tile; break; }
  if (!P->tile) {
    delete P;
    set_error("resample_plan_create: %d -> %d: a tile of %d outputs reads more than %d inputs", rate_in, rate_out, kRsThreads,
              kRsSpanMax);
    return PK2_ERR_LIMIT;
  }
  P->weights.assign((size_t)ou * max_taps, 0.f);
  P->w_dev_layout.assign((size_t)ou * max_taps, 0.f);
  P->ft_dev_layout.resize(ou);
  for (int p = 0; p < ou; ++p) {
    P->ft_dev_layout[p] = make_int2(P->first[p], P->taps[p]);
    for (int j = 0; j < P->taps[p]; ++j) {
      P->weights[(size_t)p * max_taps + j] = rows[p][j];
      P->w_dev_layout[(size_t)j * ou + p] = rows[p][j];
    }
  }
  *plan_out = P;
  return PK2_OK;
}

static size_t rs_ft_bytes(const pk2_resample_plan& P) { return align_up(P.ft_dev_layout.size() * sizeof(int2), 256); }
static size_t rs_table_bytes(const pk2_resample_plan& P) { return rs_ft_bytes(P) + P.w_dev_layout.size() * sizeof(float); }

extern "C" int pk2_resample_plan_destroy(pk2_resample_plan* plan) {
  if (!plan) return PK2_OK;
  int cur = -1;
  for (int d = 0; d < PerDevice<int>::kMax; ++d) {
    if (!plan->dev_block[d]) continue;
    if (cur < 0) PK2_HIP(hipGetDevice(&cur));
    PK2_HIP(hipSetDevice(d));
    PK2_HIP(hipFree(plan->dev_block[d]));
    plan->dev_block[d] = nullptr;
  }
  if (cur >= 0) PK2_HIP(hipSetDevice(cur));
  delete plan;
  return PK2_OK;
}

extern "C" int pk2_resample_plan_info(const pk2_resample_plan* plan, int32_t* iu, int32_t* ou, int32_t* max_taps, int32_t* tile,
                                      int64_t* table_bytes) {
  PK2_REQUIRE(plan, "resample_plan_info: null pointer");
  if (iu) *iu = plan->iu;
  if (ou) *ou = plan->ou;
  if (max_taps) *max_taps = plan->max_taps;
  if (tile) *tile = plan->tile;
  if (table_bytes) *table_bytes = (int64_t)rs_table_bytes(*plan);
  return PK2_OK;
}

extern "C" int pk2_resample_plan_export(const pk2_resample_plan* plan, int32_t* first, int32_t* taps, float* weights) {
  PK2_REQUIRE(plan && first && taps && weights, "resample_plan_export: null pointer");
  memcpy(first, plan->first.data(), plan->first.size() * sizeof(int32_t));
  memcpy(taps, plan->taps.data(), plan->taps.size() * sizeof(int32_t));
  memcpy(weights, plan->weights.data(), plan->weights.size() * sizeof(float));
  return PK2_OK;
}

extern "C" int64_t pk2_resample_num_output(const pk2_resample_plan* plan, int64_t n_in) {
  if (!plan || n_in < 0) {
    set_error("resample_num_output: null pointer or negative length");
    return -1;
  }
  const unsigned __int128 num = (unsigned __int128)n_in * (unsigned)plan->rate_out + (unsigned)plan->rate_in - 1;
  const unsigned __int128 q = num / (unsigned)plan->rate_in;
  if (q > (unsigned __int128)INT64_MAX) {
    set_error("resample_num_output: the output length does not fit 64 bits");
    return -1;
  }
  return (int64_t)q;
}

// The plan's tables on the current device; the first launch there uploads them (blocking copy: done before any later launch).
static int rs_device_tables(pk2_resample_plan* P, const int2** ft, const float** w) {
  const int dev = current_device() & (PerDevice<int>::kMax - 1);
  std::lock_guard<std::mutex> lock(P->mu);
  if (!P->dev_block[dev]) {
    void* blk = nullptr;
    PK2_HIP(hipMalloc(&blk, rs_table_bytes(*P)));
    hipError_t e = hipMemcpy(blk, P->ft_dev_layout.data(), P->ft_dev_layout.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = hipMemcpy(static_cast<char*>(blk) + rs_ft_bytes(*P), P->w_dev_layout.data(), P->w_dev_layout.size() * sizeof(float),
                    hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(blk);
      set_error("resample_batch: uploading a plan -> %s", hipGetErrorString(e));
      return PK2_ERR_HIP;
    }
    P->dev_block[dev] = blk;
  }
  *ft = static_cast<const int2*>(P->dev_block[dev]);
  *w = reinterpret_cast<const float*>(static_cast<const char*>(P->dev_block[dev]) + rs_ft_bytes(*P));
  return PK2_OK;
}

static int g_rs_last_path = PK2_RESAMPLE_PATH_NONE;

extern "C" int pk2_resample_last_path(int32_t* path) {
  PK2_REQUIRE(path, "resample_last_path: null pointer");
  *path = g_rs_last_path;
  return PK2_OK;
}

extern "C" int pk2_resample_batch(const pk2_resample_job* jobs, int32_t njobs, void* stream_) {
  PK2_REQUIRE(jobs && njobs > 0 && njobs <= PK2_RESAMPLE_MAX_JOBS, "resample_batch: bad arguments (1 <= jobs <= %d)",
              PK2_RESAMPLE_MAX_JOBS);
  const char* force = getenv("PK2_RESAMPLE_WEIGHTS");
  const bool force_mem = force && !strcmp(force, "mem");
  RsJobs tab;
  memset(&tab, 0, sizeof(tab));
  tab.njobs = njobs;
  int64_t tiles = 0;
  int path = PK2_RESAMPLE_PATH_NONE;
  for (int i = 0; i < njobs; ++i) {
    const pk2_resample_job& j = jobs[i];
    PK2_REQUIRE(j.plan && j.in && j.out && j.n_in > 0 && j.n_out > 0, "resample_batch: job %d: bad arguments", i);
    const int64_t full = pk2_resample_num_output(j.plan, j.n_in);
    PK2_REQUIRE(full > 0 && j.n_out <= full, "resample_batch: job %d: n_out %lld beyond the %lld outputs of %lld inputs", i,
                (long long)j.n_out, (long long)full, (long long)j.n_in);
    const char *a0 = reinterpret_cast<const char*>(j.in), *a1 = a0 + j.n_in * sizeof(float);
    const char *b0 = reinterpret_cast<const char*>(j.out), *b1 = b0 + j.n_out * sizeof(float);
    PK2_REQUIRE(a1 <= b0 || b1 <= a0, "resample_batch: job %d: in and out overlap", i);
    pk2_resample_plan* P = const_cast<pk2_resample_plan*>(j.plan);
    RsJobDev& d = tab.j[i];
    const int rc = rs_device_tables(P, &d.ft, &d.w);
    if (rc != PK2_OK) return rc;
    d.in = j.in; d.out = j.out; d.n_in = j.n_in; d.n_out = j.n_out;
    d.iu = P->iu; d.ou = P->ou; d.max_taps = P->max_taps; d.tile = P->tile;
    d.gain = j.gain;
    d.w_lds = !force_mem && (int64_t)P->ou * P->max_taps <= kRsWLds && P->ou <= kRsPhaseLds;
    path |= d.w_lds ? PK2_RESAMPLE_PATH_LDS : PK2_RESAMPLE_PATH_MEM;
    PK2_REQUIRE(tiles <= INT32_MAX, "resample_batch: too many tiles");
    d.tile_begin = (int32_t)tiles;
    tiles += (j.n_out + P->tile - 1) / P->tile;
  }
  PK2_REQUIRE(tiles <= INT32_MAX, "resample_batch: too many tiles");
  hipLaunchKernelGGL(resample_batch_kernel, dim3((unsigned)tiles), dim3(kRsThreads), 0, static_cast<hipStream_t>(stream_), tab);
  PK2_LAUNCH_CHECK();
  g_rs_last_path = path;
  return PK2_OK;
}
