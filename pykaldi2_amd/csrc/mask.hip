// Ideal time-frequency masks from parallel clean / distorted spectra on the device: the reference's MaskEstimator
// (simulation/mask.py:23-83).  Nothing here reads back to the host.
//
//   pk2_mask_power             P_c = |C|^2 of the clean spectra, the array the threshold passes read
//   pk2_mask_count_threshold   the cutoff of the 'count' clean mask (:75-79): sort ascending, cumulative sum, v* = the last
//                              sorted value whose inclusive cumulative sum is < (1 - 0.997) * total, mask = power > v*
//   pk2_mask_ibm               all S sources against one distorted spectrum in one launch: the SNR decision (or the soft
//                              mask) times the clean-mask decision times an optional per-frame VAD
//
// The cutoff needs no sort: a radix descent over the float32 bit pattern (non-negative floats order as unsigned ints),
// 8 bits per level.  A level builds, for the elements that share the prefix chosen so far, a histogram of
// (count, float64 sum) per bucket -- atomics in LDS, workgroup partials written out and combined in a fixed order -- and
// one thread walks the buckets in ascending order to the one in which the running sum crosses tau.
//
// The result does not depend on the order in which the atomics arrive.  A bucket of the first level (top 8 bits = sign
// + 7 exponent bits) spans two binades: its members are multiples of one ulp 2^(e-23) below 2^(e+2), so up to 2^27 of
// them sum EXACTLY in float64 (24 + 1 + 27 <= 53 bits), and the buckets of the deeper levels are narrower.  Exact sums
// are the same bits in any order; hence the limit m <= 2^27.  The sums ACROSS buckets round, but they are taken by one
// thread in ascending order.
//
// Last level: all members of the crossing bucket equal one value v, with the prefix sum s before them.  If s + v < tau the
// first copy of v still satisfies the inequality: v* = v ("strict": keep power > v).  Otherwise v* is v's predecessor,
// which is "keep power >= v".  When no element satisfies the inequality (one element; tau = 0) the reference raises
// IndexError; here the answer is (min, non-strict), an all-ones clean mask.  The decision needs (v, strict) only; v* itself
// is written beside them for whoever wants the reference's number: one more pass takes the largest element below v
// (atomicMax over the bit pattern: exact, order-independent).
#include <float.h>

#include <algorithm>

#include "common.h"

namespace pk2 {

constexpr int kMaskGroups = 64;          // workgroups per source at most (partials per level)
constexpr int kMaskPerThread = 16;       // elements per thread before another workgroup is added

// per-source state of the descent, in the workspace
struct MaskSel {
  double tau;         // (1 - energy threshold) * total
  double run;         // sum of all elements below the chosen prefix
  uint32_t prefix;    // the bits chosen so far (right-aligned)
  uint32_t pad;
};

// |z|^2 with fixed roundings: the threshold passes and the mask kernel must see the same bits
__device__ __forceinline__ float power_of(float2 z) { return __fmaf_rn(z.x, z.x, __fmul_rn(z.y, z.y)); }

__global__ void __launch_bounds__(256) mask_power_kernel(const float2* __restrict__ spec, int64_t count, float* __restrict__ power) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) power[i] = power_of(spec[i]);
}

// level in 0 .. 3: bucket = bits [31 - 8 level, 24 - 8 level] of the elements whose higher bits equal sel.prefix
__global__ void __launch_bounds__(256) mask_hist_kernel(const float* __restrict__ power, int64_t m, int level,
                                                        const MaskSel* __restrict__ sel, double* __restrict__ psum,
                                                        uint32_t* __restrict__ pcnt) {
  __shared__ double s_sum[256];
  __shared__ uint32_t s_cnt[256];
  const int src = blockIdx.y;
  s_sum[threadIdx.x] = 0.0;
  s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * level;
  const uint32_t prefix = level ? sel[src].prefix : 0u;
  const float* __restrict__ p = power + (int64_t)src * m;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const float v = p[i];
    const uint32_t u = __float_as_uint(v);
    if (level == 0 || (u >> (shift + 8)) == prefix) {
      const int b = (int)((u >> shift) & 255u);
      atomicAdd(&s_sum[b], (double)v);              // exact (see above): the arrival order does not show
      atomicAdd(&s_cnt[b], 1u);
    }
  }
  __syncthreads();
  const int64_t o = ((int64_t)src * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
  psum[o] = s_sum[threadIdx.x];
  pcnt[o] = s_cnt[threadIdx.x];
}

// one workgroup per source: thread b combines bucket b over the workgroups in order, thread 0 walks the buckets
__global__ void __launch_bounds__(256) mask_select_kernel(int level, int groups, double frac, const double* __restrict__ psum,
                                                          const uint32_t* __restrict__ pcnt, MaskSel* __restrict__ sel,
                                                          float* __restrict__ out) {
  __shared__ double s_sum[256];
  __shared__ uint32_t s_cnt[256];
  const int src = blockIdx.x;
  double sum = 0.0;
  uint32_t cnt = 0u;
  for (int g = 0; g < groups; ++g) {
    const int64_t o = ((int64_t)src * groups + g) * 256 + threadIdx.x;
    sum += psum[o];
    cnt += pcnt[o];
  }
  s_sum[threadIdx.x] = sum;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x != 0) return;
  MaskSel st = sel[src];
  if (level == 0) {
    double total = 0.0;
    for (int b = 0; b < 256; ++b) total += s_sum[b];
    st.tau = frac * total;
    st.run = 0.0;
    st.prefix = 0u;
  }
  // the first non-empty bucket whose end the running sum does not stay below tau at; the last non-empty one if the sum
  // stays below tau to the end (an energy threshold <= 0: every element satisfies the inequality)
  int pick = -1;
  double run = st.run, before = st.run;
  for (int b = 0; b < 256; ++b) {
    if (s_cnt[b] == 0u) continue;
    pick = b;
    before = run;
    if (!(run + s_sum[b] < st.tau)) break;
    run += s_sum[b];
  }
  if (pick < 0) pick = 0;                            // (m >= 1: cannot happen at level 0; deeper prefixes hold elements)
  st.run = before;
  st.prefix = (st.prefix << 8) | (uint32_t)pick;
  sel[src] = st;
  if (level == 3) {
    const float v = __uint_as_float(st.prefix);
    const bool strict = before + (double)v < st.tau;
    out[3 * src] = v;
    out[3 * src + 1] = strict ? 1.f : 0.f;
    out[3 * src + 2] = strict ? v : 0.f;              // v*; not strict: mask_pred_kernel raises it to v's predecessor
  }
}

// out[3 src + 2] = max(out[3 src + 2], the largest element below v): non-negative floats order as their bit patterns.
// Strict sources hold v there already, which no element below v exceeds.
__global__ void __launch_bounds__(256) mask_pred_kernel(const float* __restrict__ power, int64_t m, float* out) {
  const int src = blockIdx.y;
  const uint32_t vbits = __float_as_uint(out[3 * src]);
  const float* __restrict__ p = power + (int64_t)src * m;
  uint32_t best = 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const uint32_t u = __float_as_uint(p[i]);
    if (u < vbits) best = max(best, u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
  if ((threadIdx.x & 63) == 0 && best != 0u) atomicMax(reinterpret_cast<uint32_t*>(out) + 3 * src + 2, best);
}

// mask (S, N, F); clean (S, N, F) and distorted (N, F) spectra; thr (S, 3) = (v, strict, v*) or NULL; vad (N) or NULL
template <bool kSoft>
__global__ void __launch_bounds__(256) mask_ibm_kernel(const float2* __restrict__ clean, const float2* __restrict__ distorted,
                                                       int64_t m, int bins, float snr_factor, const float* __restrict__ thr,
                                                       const float* __restrict__ vad, float* __restrict__ mask) {
  const int src = blockIdx.y;
  float v = 0.f;
  bool strict = false;
  if (thr) {
    v = thr[3 * src];
    strict = thr[3 * src + 1] != 0.f;
  }
  const float2* __restrict__ C = clean + (int64_t)src * m;
  float* __restrict__ o = mask + (int64_t)src * m;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const float2 c = C[i], d = distorted[i];
    const float pc = power_of(c);
    float r;
    if (kSoft) {
      r = fminf(1.f, pc / power_of(d));              // (fminf: 0 / 0 gives 1, never NaN)
    } else {
      const float pn = power_of(make_float2(d.x - c.x, d.y - c.y));
      r = pc > snr_factor * fmaxf(pn, FLT_EPSILON) ? 1.f : 0.f;      // 10 log10(pc / max(pn, eps)) > threshold
    }
    const bool keep = !thr || (strict ? pc > v : pc >= v);
    const bool voiced = !vad || vad[i / bins] > 0.5f;
    o[i] = keep && voiced ? r : 0.f;
  }
}

static unsigned mask_groups(int64_t m, int cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (m + 256 * kMaskPerThread - 1) / (256 * kMaskPerThread)));
}

}  // namespace pk2

using namespace pk2;

extern "C" int pk2_mask_power(const float* spec, int64_t count, float* power, void* stream_) {
  PK2_REQUIRE(spec && power && count > 0, "mask_power: bad arguments");
  hipLaunchKernelGGL(mask_power_kernel, dim3(mask_groups(count, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                     reinterpret_cast<const float2*>(spec), count, power);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" size_t pk2_mask_count_workspace_bytes(int32_t S) {
  if (S < 1) return 0;
  Carver c(nullptr);
  c.take<MaskSel>((size_t)S);
  c.take<double>((size_t)S * kMaskGroups * 256);
  c.take<uint32_t>((size_t)S * kMaskGroups * 256);
  return c.bytes();
}

extern "C" int pk2_mask_count_threshold(const float* power, int32_t S, int64_t m, double energy_threshold, void* work,
                                        size_t work_bytes, float* out, void* stream_) {
  PK2_REQUIRE(power && work && out && S > 0 && S <= 65535, "mask_count_threshold: bad arguments");
  PK2_REQUIRE(m >= 1 && m <= ((int64_t)1 << 27), "mask_count_threshold: m = %lld is not in [1, 2^27] (the exact float64 sums)",
              (long long)m);
  PK2_REQUIRE(work_bytes >= pk2_mask_count_workspace_bytes(S), "mask_count_threshold: workspace of %zu bytes, %zu needed",
              work_bytes, pk2_mask_count_workspace_bytes(S));
  Carver c(work);
  MaskSel* sel = c.take<MaskSel>((size_t)S);
  double* psum = c.take<double>((size_t)S * kMaskGroups * 256);
  uint32_t* pcnt = c.take<uint32_t>((size_t)S * kMaskGroups * 256);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned groups = mask_groups(m, kMaskGroups);
  const double frac = 1.0 - energy_threshold;        // as the reference writes it
  for (int level = 0; level < 4; ++level) {
    hipLaunchKernelGGL(mask_hist_kernel, dim3(groups, (unsigned)S), dim3(256), 0, stream, power, m, level, sel, psum, pcnt);
    PK2_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_select_kernel, dim3((unsigned)S), dim3(256), 0, stream, level, (int)groups, frac, psum, pcnt, sel, out);
    PK2_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mask_pred_kernel, dim3(groups, (unsigned)S), dim3(256), 0, stream, power, m, out);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}

extern "C" int pk2_mask_ibm(const float* clean, const float* distorted, int32_t S, int32_t N, int32_t F, float snr_factor,
                            int32_t soft, const float* thr, const float* vad, float* mask, void* stream_) {
  PK2_REQUIRE(clean && distorted && mask && S > 0 && S <= 65535 && N > 0 && F > 0, "mask_ibm: bad arguments");
  const int64_t m = (int64_t)N * F;
  const dim3 grid(mask_groups(m, 1024), (unsigned)S);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const float2* C = reinterpret_cast<const float2*>(clean);
  const float2* D = reinterpret_cast<const float2*>(distorted);
  if (soft)
    hipLaunchKernelGGL(mask_ibm_kernel<true>, grid, dim3(256), 0, stream, C, D, m, F, snr_factor, thr, vad, mask);
  else
    hipLaunchKernelGGL(mask_ibm_kernel<false>, grid, dim3(256), 0, stream, C, D, m, F, snr_factor, thr, vad, mask);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
