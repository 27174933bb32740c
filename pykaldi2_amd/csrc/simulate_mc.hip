// Multi-channel, multi-source simulation of one utterance on the device: the arithmetic of the reference's
// _Simulator.simulate (simulation/simulation.py:55-178) beyond one source and one channel -- Distorter.apply_rir with a
// (T, C) RIR and its early-reverberation output (_distorter.py:119-154), Mixer.mix_signals (_mixer.py:29-107),
// Distorter.add_noise with both placements over C channels (_distorter.py:33-117) and the gain normalisation of the
// mixture and the early-reverberation signals (simulation.py:171-176).  Device layout: channel-major, (C, T).
//
//   pk2_sim_apply_rir_mc   all (source, channel) rows of an utterance in one launch, optional early reverberation
//   pk2_sim_power_seg      sum of squares (float64) and max |x| of every source in one launch
//   pk2_sim_mix            source scales from the power buffers, placement at the start samples, the sum
//   pk2_sim_add_noise_mc   noise at an SNR over C rows, 'sample_noise' and 'repeat_noise' placement
//   pk2_sim_gain_norm_seg  0.5 / max|x| applied to several buffers
// The small tables (jobs, segments, sources: at most PK2_SIM_MAX_SEGS entries) travel as kernel arguments, so a call
// uploads nothing; statistics, scales and delays stay in device memory.
#include <algorithm>

#include "common.h"
#include "sim_tile.h"

namespace pk2 {

struct RirJobs { pk2_sim_rir_job j[PK2_SIM_MAX_SEGS]; };
struct Segs { pk2_sim_seg s[PK2_SIM_MAX_SEGS]; };
struct MixSrcs { pk2_sim_mix_src s[PK2_SIM_MAX_SEGS]; };

// grid (tiles of the longest source, channels, sources).  Every row of a source is shifted by the delay of the
// source's channel 0 (the reference: int(np.argmax(rir, axis=0)[0])).
__global__ void __launch_bounds__(kSimThreads) sim_apply_rir_mc_kernel(const RirJobs jobs, int early_taps) {
  PK2_SIM_TILE_LDS;
  const pk2_sim_rir_job& jb = jobs.j[blockIdx.z];
  const int64_t n = jb.n;
  if ((int64_t)blockIdx.x * kSimTile >= n) return;          // uniform over the workgroup
  const int k = jb.k, c = blockIdx.y;
  const int d = jb.delay_dev ? min(max(*jb.delay_dev, 0), k - 1) : jb.delay;
  const int64_t base = d > 0 ? d - 1 : 0;
  const float* rir = jb.rir + (int64_t)c * k;
  if (jb.early) sim_apply_rir_tile<true>(jb.wav, n, rir, k, base, jb.out + c * n, blockIdx.x, s_rir, s_wav,
                                            jb.early + c * n, min(k, early_taps + d));
  else sim_apply_rir_tile<false>(jb.wav, n, rir, k, base, jb.out + c * n, blockIdx.x, s_rir, s_wav);
}

// grid (blocks, segments): sim_power_kernel per segment
__global__ void __launch_bounds__(256) sim_power_seg_kernel(const Segs segs, double* stats) {
  __shared__ double s_sum[4];
  __shared__ float s_max[4];
  const float* __restrict__ x = segs.s[blockIdx.y].x;
  const int64_t n = segs.s[blockIdx.y].count;
  double sum = 0.0;
  float mx = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    sum += (double)v * (double)v;
    mx = fmaxf(mx, fabsf(v));
  }
  sum = wave_sum_d(sum);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_max[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* st = stats + 2 * blockIdx.y;
    atomicAdd(&st[0], s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
    const double m = (double)fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    // non-negative doubles order like their bit patterns
    atomicMax(reinterpret_cast<unsigned long long*>(&st[1]), (unsigned long long)__double_as_longlong(m));
  }
}

__global__ void __launch_bounds__(256) sim_gain_norm_seg_kernel(const Segs segs, const double* stats, double* gain) {
  const double gd = 0.5 / stats[1];
  const float g = (float)gd;
  float* __restrict__ x = segs.s[blockIdx.y].x;
  const int64_t n = segs.s[blockIdx.y].count;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] *= g;
  if (gain && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *gain = gd;
}

// grid (blocks over T, channels).  _compute_source_scales: sqrt(P_ref / P_i * 10^(spr_i / 10)), powers = means over
// the whole (C, n_i) source; _mix_by_random_start: the sum of the placed, scaled sources in source order.
__global__ void __launch_bounds__(256) sim_mix_kernel(const MixSrcs srcs, int nsrc, int channels, int64_t T,
                                                      const double* __restrict__ stats, float* __restrict__ mixed,
                                                      double* __restrict__ scales) {
  __shared__ float s_scale[PK2_SIM_MAX_SEGS];
  if ((int)threadIdx.x < nsrc) {
    const int i = threadIdx.x;
    const double p_ref = stats[0] / ((double)channels * (double)srcs.s[0].n);
    const double p_i = stats[2 * i] / ((double)channels * (double)srcs.s[i].n);
    const double sc = sqrt(p_ref / p_i * pow(10.0, srcs.s[i].spr_db / 10.0));
    s_scale[i] = (float)sc;
    if (blockIdx.x == 0 && blockIdx.y == 0) scales[i] = sc;
  }
  __syncthreads();
  const int c = blockIdx.y;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256) {
    float sum = 0.f;
    for (int i = 0; i < nsrc; ++i) {
      const pk2_sim_mix_src& s = srcs.s[i];
      const int64_t u = t - s.start;
      const bool in = u >= 0 && u < s.n;
      const float v = in ? s.sig[c * s.n + u] : 0.f;
      sum += s_scale[i] * v;
      if (s.pos) s.pos[c * T + t] = v;
      if (s.pos2) s.pos2[c * T + t] = in ? s.sig2[c * s.n + u] * s_scale[i] : 0.f;
    }
    mixed[c * T + t] = sum;
  }
}

// grid (blocks over n, channels)
__global__ void __launch_bounds__(256) sim_add_noise_mc_kernel(float* __restrict__ mixed, int64_t n,
                                                               const float* __restrict__ noise, int64_t m, int channels,
                                                               int64_t start, float snr_db, int repeat,
                                                               const double* sig_stats, const double* noise_stats) {
  // _comp_noise_scale_given_snr: the means run over all channels
  const double px = sig_stats[0] / ((double)n * channels), pn = noise_stats[0] / ((double)m * channels);
  const float scale = (float)sqrt(px / pn * pow(10.0, -(double)snr_db / 10.0));
  float* __restrict__ row = mixed + blockIdx.y * n;
  const float* __restrict__ nz = noise + blockIdx.y * m;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v;
    if (repeat) v = nz[(start + i) % m];                                      // tiled noise (or a longer one) from `start`
    else if (m <= n) v = (i >= start && i < start + m) ? nz[i - start] : 0.f;   // shorter noise placed at `start`
    else v = nz[start + i];                                                     // longer noise cropped from `start`
    row[i] += scale * v;
  }
}

static inline unsigned grid_for(int64_t n, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap)); }

}  // namespace pk2

using namespace pk2;

extern "C" int pk2_sim_apply_rir_mc(const pk2_sim_rir_job* jobs, int32_t njobs, int32_t channels, int32_t early_taps,
                                    void* stream_) {
  PK2_REQUIRE(jobs && njobs > 0 && njobs <= PK2_SIM_MAX_SEGS && channels > 0 && channels <= 65535 && early_taps >= 0,
              "sim_apply_rir_mc: bad arguments (1 <= jobs <= %d)", PK2_SIM_MAX_SEGS);
  RirJobs tab;
  memset(&tab, 0, sizeof(tab));
  int64_t nmax = 0;
  for (int i = 0; i < njobs; ++i) {
    const pk2_sim_rir_job& j = jobs[i];
    PK2_REQUIRE(j.wav && j.rir && j.out && j.n > 0 && j.k > 0, "sim_apply_rir_mc: job %d: bad arguments", i);
    PK2_REQUIRE(j.delay_dev || (j.delay >= 0 && j.delay < j.k), "sim_apply_rir_mc: job %d: delay %d outside [0, %d)", i,
                j.delay, j.k);
    PK2_REQUIRE(j.wav != j.out && j.wav != j.early && j.out != j.early, "sim_apply_rir_mc: job %d: aliased arrays", i);
    tab.j[i] = j;
    nmax = std::max(nmax, j.n);
  }
  hipLaunchKernelGGL(sim_apply_rir_mc_kernel, dim3((unsigned)((nmax + kSimTile - 1) / kSimTile), (unsigned)channels, (unsigned)njobs),
                     dim3(kSimThreads), 0, static_cast<hipStream_t>(stream_), tab, early_taps);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

static int fill_segs(const pk2_sim_seg* segs, int32_t nseg, Segs* tab, int64_t* nmax, const char* who) {
  PK2_REQUIRE(segs && nseg > 0 && nseg <= PK2_SIM_MAX_SEGS, "%s: bad arguments (1 <= segments <= %d)", who, PK2_SIM_MAX_SEGS);
  memset(tab, 0, sizeof(*tab));
  *nmax = 0;
  for (int i = 0; i < nseg; ++i) {
    PK2_REQUIRE(segs[i].x && segs[i].count > 0, "%s: segment %d: bad arguments", who, i);
    tab->s[i] = segs[i];
    *nmax = std::max(*nmax, segs[i].count);
  }
  return PK2_OK;
}

extern "C" int pk2_sim_power_seg(const pk2_sim_seg* segs, int32_t nseg, double* stats, void* stream_) {
  Segs tab;
  int64_t nmax;
  if (int rc = fill_segs(segs, nseg, &tab, &nmax, "sim_power_seg")) return rc;
  PK2_REQUIRE(stats, "sim_power_seg: null stats");
  hipLaunchKernelGGL(sim_power_seg_kernel, dim3(grid_for(nmax, 1024), (unsigned)nseg), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), tab, stats);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_sim_gain_norm_seg(const pk2_sim_seg* segs, int32_t nseg, const double* stats, double* gain, void* stream_) {
  Segs tab;
  int64_t nmax;
  if (int rc = fill_segs(segs, nseg, &tab, &nmax, "sim_gain_norm_seg")) return rc;
  PK2_REQUIRE(stats, "sim_gain_norm_seg: null stats");
  hipLaunchKernelGGL(sim_gain_norm_seg_kernel, dim3(grid_for(nmax, 1024), (unsigned)nseg), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), tab, stats, gain);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_sim_mix(const pk2_sim_mix_src* srcs, int32_t nsrc, int32_t channels, int64_t T, const double* stats,
                           float* mixed, double* scales, void* stream_) {
  PK2_REQUIRE(srcs && nsrc > 0 && nsrc <= PK2_SIM_MAX_SEGS && channels > 0 && channels <= 65535 && T > 0 && stats && mixed && scales,
              "sim_mix: bad arguments (1 <= sources <= %d)", PK2_SIM_MAX_SEGS);
  MixSrcs tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 0; i < nsrc; ++i) {
    const pk2_sim_mix_src& s = srcs[i];
    PK2_REQUIRE(s.sig && s.n > 0 && (!s.pos2 || s.sig2), "sim_mix: source %d: bad arguments", i);
    PK2_REQUIRE(s.start >= 0 && s.start + s.n <= T, "sim_mix: source %d: [%lld, %lld) outside the mixture of %lld samples", i,
                (long long)s.start, (long long)(s.start + s.n), (long long)T);
    tab.s[i] = s;
  }
  hipLaunchKernelGGL(sim_mix_kernel, dim3(grid_for(T, 1024), (unsigned)channels), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), tab, nsrc, channels, T, stats, mixed, scales);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_sim_add_noise_mc(float* mixed, int64_t n, const float* noise, int64_t m, int32_t channels, int64_t start,
                                    float snr_db, int32_t repeat, const double* sig_stats, const double* noise_stats,
                                    void* stream_) {
  PK2_REQUIRE(mixed && noise && sig_stats && noise_stats && n > 0 && m > 0 && channels > 0 && channels <= 65535 &&
              (repeat == 0 || repeat == 1), "sim_add_noise_mc: bad arguments");
  if (repeat) {
    const int64_t tiled = m < n ? (n + m - 1) / m * m : m;
    PK2_REQUIRE(start >= 0 && start <= tiled - n, "sim_add_noise_mc: noise position %lld outside [0, %lld]", (long long)start,
                (long long)(tiled - n));
  } else {
    PK2_REQUIRE(start >= 0 && (m <= n ? start + m <= n : start + n <= m), "sim_add_noise_mc: noise position %lld outside its range",
                (long long)start);
  }
  hipLaunchKernelGGL(sim_add_noise_mc_kernel, dim3(grid_for(n, 1024), (unsigned)channels), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), mixed, n, noise, m, channels, start, snr_db, repeat, sig_stats,
                     noise_stats);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
