// SpecAugment on the packed feature rows of a ragged minibatch in one launch: time warp, then frequency and time masks
// in output coordinates (include/pk2hip.h).
//
// A row is 80 float32 = 20 aligned 16-byte quads and the rows lie back to back, so a tile of kSpecRows rows is one
// contiguous run of kSpecRows * 20 quads: lane i of the workgroup moves quad i, i + 256, ... of the run, neighbouring
// lanes neighbouring 16 bytes.  What a row needs -- its utterance (bisection over row_off), its frame index, whether a time
// interval covers it, the two source frames and the weight of the warp -- is worked out once per row by the first
// kSpecRows lanes and left in LDS, next to the plan rows of the tile's utterances; the quad loop reads only LDS and the
// data.  Values move as 32-bit words and only interpolated elements pass through the float unit, so every other element is
// a bit-exact copy.  No atomics, one writer per element.
#include "common.h"

namespace pk2 {

constexpr int kSpecThreads = 256;
constexpr int kSpecRows = 32;                      // rows per workgroup
constexpr int kSpecQuads = 20;                     // 16-byte quads per row (80 float32)
constexpr int kSpecPlans = kSpecRows;              // plan rows staged per tile: one per row unless utterances are empty
constexpr int kSpecFreq0 = 2;                                            // plan row: c, d, frequency pairs, time pairs
constexpr int kSpecTime0 = 2 + 2 * PK2_SPEC_MAX_FREQ_MASKS;

struct SpecRow {
  int64_t src0, src1;   // rows of `in` the output row is made of (src0 == src1 and w unused when not interpolated)
  float w;              // weight of src1
  int32_t utt;          // utterance, -1: the row lies outside every utterance (copied as it is)
  int32_t flags;        // bit 0: a time interval covers the row, bit 1: interpolated
};

// The last utterance whose first row is <= row (empty utterances share their first row with their successor and lose).
__device__ __forceinline__ int spec_find_utt(const int64_t* __restrict__ row_off, int n, int64_t row) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row_off[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ uint32_t spec_lerp(uint32_t a, uint32_t b, float w) {
  const float fa = __uint_as_float(a), fb = __uint_as_float(b);
  return __float_as_uint(fmaf(w, fb - fa, fa));
}

// kWarp: rows may be interpolated (in != out).  kInPlace: in == out, nothing is read and only masked elements are written.
template <bool kWarp, bool kInPlace>
__global__ void __launch_bounds__(kSpecThreads) spec_augment_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                                    const int64_t* __restrict__ row_off, int n,
                                                                    int64_t total_rows, const int32_t* __restrict__ plan,
                                                                    uint32_t fill) {
  __shared__ SpecRow s_row[kSpecRows];
  __shared__ int32_t s_plan[kSpecPlans * PK2_SPEC_PLAN_STRIDE];
  __shared__ int s_u0, s_u1;
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kSpecRows;
  const int nrows = (int)min((int64_t)kSpecRows, total_rows - r0);
  if (nrows <= 0) return;

  int utt = 0;
  if (tid < nrows) {
    utt = spec_find_utt(row_off, n, r0 + tid);
    if (tid == 0) s_u0 = utt;
    if (tid == nrows - 1) s_u1 = utt;
  }
  __syncthreads();
  const int u0 = s_u0, nplans = min(s_u1 - u0 + 1, kSpecPlans);
  for (int i = tid; i < nplans * PK2_SPEC_PLAN_STRIDE; i += kSpecThreads) s_plan[i] = plan[(int64_t)u0 * PK2_SPEC_PLAN_STRIDE + i];
  __syncthreads();

  if (tid < nrows) {
    const int64_t row = r0 + tid, first = row_off[utt];
    const int64_t T = row_off[utt + 1] - first, t = row - first;
    SpecRow sr;
    sr.src0 = sr.src1 = row; sr.w = 0.f; sr.utt = -1; sr.flags = 0;
    if (t >= 0 && t < T) {
      sr.utt = utt;
      const int32_t* p = utt - u0 < kSpecPlans ? s_plan + (utt - u0) * PK2_SPEC_PLAN_STRIDE
                                               : plan + (int64_t)utt * PK2_SPEC_PLAN_STRIDE;
      bool masked = false;
      for (int k = 0; k < PK2_SPEC_MAX_TIME_MASKS; ++k) masked |= t >= p[kSpecTime0 + 2 * k] && t < p[kSpecTime0 + 2 * k + 1];
      sr.flags = masked ? 1 : 0;
      if (kWarp && !masked) {
        const int64_t c = p[0], d = p[1];
        if (c != d) {
          int64_t base, num, den;
          if (t <= d) { base = 0; num = t * c; den = d; }
          else { base = c; num = (t - d) * (T - 1 - c); den = T - 1 - d; }
          if (den > 0 && num >= 0) {      // (a plan the host interface would have refused leaves the row a copy)
            const int64_t q = num / den, r = num - q * den;
            const int64_t i0 = min(max(base + q, (int64_t)0), T - 1), i1 = min(i0 + 1, T - 1);
            sr.src0 = first + i0;
            sr.src1 = r != 0 ? first + i1 : sr.src0;
            if (r != 0) { sr.w = (float)r / (float)den; sr.flags |= 2; }
          }
        }
      }
    }
    s_row[tid] = sr;
  }
  __syncthreads();

  const int nquads = nrows * kSpecQuads;
  const uint4 fill4 = make_uint4(fill, fill, fill, fill);
  for (int i = tid; i < nquads; i += kSpecThreads) {
    const int rl = i / kSpecQuads, f0 = (i - rl * kSpecQuads) * 4;
    const SpecRow sr = s_row[rl];
    const int64_t o = r0 * kSpecQuads + i;
    int m = 0;       // bit e: element f0 + e is masked
    if (sr.flags & 1) {
      m = 15;
    } else if (sr.utt >= 0) {
      const int32_t* p = sr.utt - u0 < kSpecPlans ? s_plan + (sr.utt - u0) * PK2_SPEC_PLAN_STRIDE
                                                  : plan + (int64_t)sr.utt * PK2_SPEC_PLAN_STRIDE;
#pragma unroll
      for (int k = 0; k < PK2_SPEC_MAX_FREQ_MASKS; ++k) {
        const int a = p[kSpecFreq0 + 2 * k], b = p[kSpecFreq0 + 2 * k + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) m |= (f0 + e >= a && f0 + e < b) ? 1 << e : 0;
      }
    }
    if (kInPlace) {
      if (m == 15) {
        out[o] = fill4;
      } else if (m) {
        uint32_t* w = reinterpret_cast<uint32_t*>(out + o);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m >> e & 1) w[e] = fill;
      }
      continue;
    }
    uint4 v = fill4;
    if (m != 15) {
      const int64_t q = (i - rl * kSpecQuads);
      v = in[sr.src0 * kSpecQuads + q];
      if (kWarp && (sr.flags & 2)) {
        const uint4 b = in[sr.src1 * kSpecQuads + q];
        v.x = spec_lerp(v.x, b.x, sr.w); v.y = spec_lerp(v.y, b.y, sr.w);
        v.z = spec_lerp(v.z, b.z, sr.w); v.w = spec_lerp(v.w, b.w, sr.w);
      }
      if (m & 1) v.x = fill;
      if (m & 2) v.y = fill;
      if (m & 4) v.z = fill;
      if (m & 8) v.w = fill;
    }
    out[o] = v;
  }
}

}  // namespace pk2

using namespace pk2;

extern "C" int pk2_spec_augment(const float* in, float* out, const int64_t* row_off, int32_t n, int64_t total_rows,
                                const int32_t* plan, int32_t has_warp, float fill, void* stream_) {
  PK2_REQUIRE(in && out && row_off && plan, "spec_augment: null pointer");
  PK2_REQUIRE(n >= 1 && total_rows >= n, "spec_augment: bad arguments (n %d >= 1, total_rows %lld >= n)", n, (long long)total_rows);
  PK2_REQUIRE((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0,
              "spec_augment: in and out must be 16-byte aligned");
  PK2_REQUIRE(!(has_warp && in == out), "spec_augment: a warping plan cannot run in place (in == out with has_warp != 0)");
  const int64_t blocks = (total_rows + kSpecRows - 1) / kSpecRows;
  PK2_REQUIRE(blocks <= INT32_MAX, "spec_augment: too many rows (%lld)", (long long)total_rows);
  if (in != out) {
    const char *a0 = reinterpret_cast<const char*>(in), *b0 = reinterpret_cast<const char*>(out);
    const int64_t bytes = total_rows * kSpecQuads * 16;
    PK2_REQUIRE(a0 + bytes <= b0 || b0 + bytes <= a0, "spec_augment: in and out overlap without being equal");
  }
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, sizeof(fill_bits));
  const uint4* in4 = reinterpret_cast<const uint4*>(in);
  uint4* out4 = reinterpret_cast<uint4*>(out);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 grid((unsigned)blocks), block(kSpecThreads);
  if (in == out)
    hipLaunchKernelGGL((spec_augment_kernel<false, true>), grid, block, 0, stream, in4, out4, row_off, n, total_rows, plan, fill_bits);
  else if (has_warp)
    hipLaunchKernelGGL((spec_augment_kernel<true, false>), grid, block, 0, stream, in4, out4, row_off, n, total_rows, plan, fill_bits);
  else
    hipLaunchKernelGGL((spec_augment_kernel<false, false>), grid, block, 0, stream, in4, out4, row_off, n, total_rows, plan, fill_bits);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
