// Room impulse responses by the image method on the device: the arithmetic of the reference's
// simulation/_rirgen.py `xp_rirgen(method=1)` (image lattice candidates, the 8 side combinations per lattice point,
// the Hann-windowed sinc spread of every image, the FIR or Habets high-pass), for a batch of items in one call.
//
//   rirgen_taps_kernel      one workgroup per (row, part of the row's image lattice, segment of the row's samples).
//                           A thread takes lattice points (z fastest), applies the reference's rough candidate rule,
//                           forms the 8 images of a kept point in double and spreads their taps into the segment,
//                           held in LDS as 64-bit fixed point (tap * 2^40).  The segment is then added into the row's
//                           global fixed-point accumulator.
//   rirgen_finish_kernel    one workgroup per row: fixed point -> f32 (the value the reference's float32 scatter-add
//                           holds), the high-pass, the f32 row, and the row's argmax (the `delay` of
//                           Distorter.apply_rir).
//
// Bit reproducibility: every sum is an integer sum, so its result does not depend on the order in which the images
// arrive (LDS and global 64-bit integer atomics), while a float atomic sum would.  The fixed point quantum, 2^-40,
// is about 1e-12: far below the float32 rounding of a tap (the reference rounds each tap to f32 and sums in f32).
#include "common.h"

namespace pk2 {

constexpr int kRirThreads = 256;
constexpr int kRirSeg = 8192;          // samples per LDS segment: 64 KB of int64 (a T60 <= 0.512 s row is one segment)
constexpr double kRirFix = 0x1p40;     // fixed point scale of a tap

struct RirItem {                        // one item, decoded from the f64 / i64 descriptor rows (include/pk2hip.h)
  double room[3], beta[6], c0, thr, cts, hb1, hb2, ha1, ha2;
  int64_t nsrc, nmic, ns, htw, mode, pos, out, row0, ax, ay, az;
};

__device__ inline RirItem load_item(const double* f, const int64_t* n, int item) {
  RirItem it;
  const double* fi = f + (int64_t)item * PK2_RIR_F64;
  const int64_t* ni = n + (int64_t)item * PK2_RIR_I64;
  for (int q = 0; q < 3; ++q) it.room[q] = fi[q];
  for (int q = 0; q < 6; ++q) it.beta[q] = fi[3 + q];
  it.c0 = fi[9]; it.thr = fi[10]; it.cts = fi[11];
  it.hb1 = fi[12]; it.hb2 = fi[13]; it.ha1 = fi[14]; it.ha2 = fi[15];
  it.nsrc = ni[0]; it.nmic = ni[1]; it.ns = ni[2]; it.htw = ni[3]; it.mode = ni[4]; it.pos = ni[5]; it.out = ni[6];
  it.row0 = ni[7]; it.ax = ni[8]; it.ay = ni[9]; it.az = ni[10];
  return it;
}

// wg[b] = {item, row within the item (src * nmic + mic), part, number of parts, first sample of the segment}
__global__ void __launch_bounds__(kRirThreads) rirgen_taps_kernel(const double* __restrict__ item_f64,
                                                                  const int64_t* __restrict__ item_i64,
                                                                  const double* __restrict__ pos,
                                                                  const int32_t* __restrict__ wg,
                                                                  unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long seg[kRirSeg];
  const int32_t* w = wg + (int64_t)blockIdx.x * 5;
  const RirItem it = load_item(item_f64, item_i64, w[0]);
  const int rowi = w[1], part = w[2], nparts = w[3];
  const int64_t seg0 = w[4];
  const int64_t seg_len = min((int64_t)kRirSeg, it.ns - seg0);
  const int tid = threadIdx.x;
  for (int64_t j = tid; j < seg_len; j += kRirThreads) seg[j] = 0ull;
  __syncthreads();

  const int src = rowi / (int)it.nmic, mic = rowi % (int)it.nmic;
  const double* ps = pos + it.pos + 3 * (int64_t)src;
  const double* pm = pos + it.pos + 3 * (it.nsrc + mic);
  const double sx = ps[0], sy = ps[1], sz = ps[2], mx = pm[0], my = pm[1], mz = pm[2];
  const double bx = it.beta[0] * it.beta[1], by = it.beta[2] * it.beta[3], bz = it.beta[4] * it.beta[5];
  const int64_t ly = 2 * it.ay + 1, lz = 2 * it.az + 1, npts = (2 * it.ax + 1) * ly * lz;
  const int htw = (int)it.htw;
  const double dmax = (double)(it.ns - it.htw - 2);
  const float inv_htw = htw > 0 ? 1.0f / (float)htw : 0.f;
  const int64_t lo = seg0, hi = seg0 + seg_len;             // taps kept here: [lo, hi)

  // part `part` of `nparts` takes the lattice points [p0, p1), consecutive threads on consecutive z
  const int64_t per = (npts + nparts - 1) / nparts;
  const int64_t p0 = (int64_t)part * per, p1 = min(npts, p0 + per);
  for (int64_t p = p0 + tid; p < p1; p += kRirThreads) {
    const int64_t x = p / (ly * lz) - it.ax, y = (p / lz) % ly - it.ay, z = p % lz - it.az;
    // get_reflection_candidates: rough delay from the origin and rough gain, src-mic distance taken as 0.5 m
    const double rx = (double)(2 * x) * it.room[0], ry = (double)(2 * y) * it.room[1], rz = (double)(2 * z) * it.room[2];
    const double rd = sqrt(rx * rx + ry * ry + rz * rz);
    const double rg = pow(bx, (double)llabs(x)) * pow(by, (double)llabs(y)) * pow(bz, (double)llabs(z)) / (rd + it.c0);
    if (!(rd < (double)it.ns && rg > it.thr)) continue;
    const double b1x = pow(it.beta[1], (double)llabs(x)), b1y = pow(it.beta[3], (double)llabs(y)),
                 b1z = pow(it.beta[5], (double)llabs(z));
    for (int side = 0; side < 8; ++side) {
      const int ex = side >> 2, ey = (side >> 1) & 1, ez = side & 1;
      // get_delays_and_gains
      const double dx = ((double)(2 * x) * it.room[0] - mx) + (double)(1 - 2 * ex) * sx;
      const double dy = ((double)(2 * y) * it.room[1] - my) + (double)(1 - 2 * ey) * sy;
      const double dz = ((double)(2 * z) * it.room[2] - mz) + (double)(1 - 2 * ez) * sz;
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      if (!(d < dmax)) continue;
      const double refl = (pow(it.beta[0], (double)llabs(x - ex)) * b1x) * (pow(it.beta[2], (double)llabs(y - ey)) * b1y) *
                          (pow(it.beta[4], (double)llabs(z - ez)) * b1z);
      const float g = (float)(refl / (4.0 * M_PI * d * it.cts));
      const double fl = floor(d), frac = d - fl;
      const int64_t base = (int64_t)fl - htw + 1;             // tap k lands on sample base + k
      const int k0 = (int)max((int64_t)0, lo - base), k1 = (int)min((int64_t)(2 * htw), hi - base);
      // sin(pi (1 - frac + k - htw)) = (-1)^(k - htw) sin(pi frac): one sine per image
      const float sp = (float)sin(M_PI * frac);
#pragma unroll 4
      for (int k = k0; k < k1; ++k) {
        const double t = ((1.0 - frac) + (double)k) - (double)htw;     // garg / pi, formed like the reference
        const float garg = (float)(M_PI * t);
        const float win = 0.5f * (1.0f + cosf(garg * inv_htw));         // 0.5 (1 - cos(pi + garg / htw))
        const float sinc = t == 0.0 ? 1.0f : (((k - htw) & 1) ? -sp : sp) / garg;
        const float tap = g * win * sinc;
        const long long q = llrint((double)tap * kRirFix);
        if (q != 0) atomicAdd(&seg[base + k - seg0], (unsigned long long)q);
      }
    }
  }
  __syncthreads();
  unsigned long long* row = acc + it.out + (int64_t)rowi * it.ns + seg0;
  for (int64_t j = tid; j < seg_len; j += kRirThreads) {
    const unsigned long long v = seg[j];
    if (v != 0ull) atomicAdd(&row[j], v);
  }
}

__device__ inline float fix_to_f32(unsigned long long v) { return (float)((double)(long long)v * (1.0 / kRirFix)); }

__global__ void __launch_bounds__(kRirThreads) rirgen_finish_kernel(const double* __restrict__ item_f64,
                                                                    const int64_t* __restrict__ item_i64,
                                                                    const int32_t* __restrict__ row_item,
                                                                    const unsigned long long* __restrict__ acc,
                                                                    float* __restrict__ out, int32_t* __restrict__ delay) {
  __shared__ float s_val[kRirThreads / 64];
  __shared__ int s_idx[kRirThreads / 64];
  const int item = row_item[2 * blockIdx.x], rowi = row_item[2 * blockIdx.x + 1];
  const RirItem it = load_item(item_f64, item_i64, item);
  const int64_t n = it.ns, off = it.out + (int64_t)rowi * n;
  const unsigned long long* a = acc + off;
  float* o = out + off;
  const int tid = threadIdx.x;
  if (it.mode == 2) {
    // Habets' high-pass: scipy.signal.lfilter(b, a, rir) (transposed direct form II, double state) over the f32 RIR
    if (tid == 0) {
      double z0 = 0.0, z1 = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        const double x = (double)fix_to_f32(a[i]);
        const double y = z0 + x;                                         // b0 = 1
        z0 = (z1 + x * it.hb1) - y * it.ha1;
        z1 = x * it.hb2 - y * it.ha2;
        o[i] = (float)y;
      }
    }
    __threadfence_block();
    __syncthreads();
  } else {
    for (int64_t i = tid; i < n; i += kRirThreads) {
      float v = fix_to_f32(a[i]);
      if (it.mode == 1 && i > 0 && i < n - 1) {
        // rirs[1:-1] += -0.5 * rirs[2:] - 0.5 * rirs[:-2]  (float32, right-hand side from the unfiltered values)
        const float t = (-0.5f * fix_to_f32(a[i + 1])) - (0.5f * fix_to_f32(a[i - 1]));
        v = v + t;
      }
      o[i] = v;
    }
    __threadfence_block();
    __syncthreads();
  }
  // argmax, first index of the maximum (np.argmax / torch.argmax)
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int64_t i = tid; i < n; i += kRirThreads) {
    const float v = o[i];
    if (v > best) { best = v; bi = (int)i; }
  }
  for (int m = 32; m > 0; m >>= 1) {
    const float ov = __shfl_xor(best, m);
    const int oi = __shfl_xor(bi, m);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { s_val[tid >> 6] = best; s_idx[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < kRirThreads / 64; ++q)
      if (s_val[q] > best || (s_val[q] == best && s_idx[q] < bi)) { best = s_val[q]; bi = s_idx[q]; }
    delay[it.row0 + rowi] = bi == 0x7fffffff ? 0 : bi;
  }
}

}  // namespace pk2

using namespace pk2;

extern "C" int32_t pk2_rirgen_segment_samples(void) { return kRirSeg; }

extern "C" int pk2_rirgen(const double* item_f64, const int64_t* item_i64, const double* pos, const int32_t* wg,
                          int32_t nwg, const int32_t* row_item, int32_t nrows, int64_t total, void* acc, float* out,
                          int32_t* delay, void* stream_) {
  PK2_REQUIRE(item_f64 && item_i64 && pos && wg && row_item && acc && out && delay, "rirgen: null pointer");
  PK2_REQUIRE(nwg > 0 && nrows > 0 && total > 0, "rirgen: empty batch");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  PK2_HIP(hipMemsetAsync(acc, 0, (size_t)total * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(rirgen_taps_kernel, dim3((unsigned)nwg), dim3(kRirThreads), 0, stream, item_f64, item_i64, pos, wg,
                     static_cast<unsigned long long*>(acc));
  PK2_LAUNCH_CHECK();
  hipLaunchKernelGGL(rirgen_finish_kernel, dim3((unsigned)nrows), dim3(kRirThreads), 0, stream, item_f64, item_i64,
                     row_item, static_cast<const unsigned long long*>(acc), out, delay);
  PK2_LAUNCH_CHECK();
  return PK2_OK;
}
