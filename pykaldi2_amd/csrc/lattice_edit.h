// Levenshtein distance with unit costs on one wavefront, shared by the MWE loss (lattice_nbest.hip: mwe_edit) and the
// scoring tools (lattice_score.hip: ws_edit_kernel).
#pragma once
#include "common.h"

namespace pk2 {

constexpr int kEdChunks = 16;          // Levenshtein: a second sequence of at most 64 * 16 - 1 labels

// Distance of x[0..a) and y[0..b), b <= 64 * kEdChunks - 1, returned in every lane: rows = the labels of x, the row of DP
// values over the positions j = 0..b of y held by the lanes (j = 64 c + lane), the insertion chain as a prefix minimum.
__device__ __forceinline__ int edit_wave(const int32_t* x, int a, const int32_t* y, int b, int lane) {
  const int nc = b / 64 + 1;
  int prev[kEdChunks], ylab[kEdChunks];
#pragma unroll
  for (int c = 0; c < kEdChunks; ++c) {
    const int j = 64 * c + lane;
    prev[c] = j;
    ylab[c] = (c < nc && j >= 1 && j <= b) ? y[j - 1] : 0;
  }
  for (int i = 1; i <= a; ++i) {
    const int xi = x[i - 1];
    int carry_old = 0, carry_min = 0x3FFFFFFF;
#pragma unroll
    for (int c = 0; c < kEdChunks; ++c) {
      if (c < nc) {
        const int j = 64 * c + lane;
        const int up = prev[c];
        int diag = __shfl_up(up, 1, 64);
        if (lane == 0) diag = carry_old;
        const int tmp = j == 0 ? i : min(up + 1, diag + (xi != ylab[c] ? 1 : 0));
        int v = tmp - j;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v = min(v, u); }
        v = min(v, carry_min);
        carry_old = __shfl(up, 63, 64);
        carry_min = __shfl(v, 63, 64);
        prev[c] = v + j;
      }
    }
  }
  int e = 0;
#pragma unroll
  for (int c = 0; c < kEdChunks; ++c) if (c == b / 64) e = prev[c];
  return __shfl(e, b % 64, 64);
}

}  // namespace pk2
