// The packed descriptor and the workspace layout of the transducer's first stage (csrc/transducer.hip), shared with the
// pruning ranges of csrc/transducer_pruned.hip, which read the occupancies that the first stage left in its workspace.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace pk2td {

// Packed descriptor (int32 words, made by pykaldi2_amd/transducer.py): N of these, then per utterance its labels [U], the
// label positions 0..U-1 sorted by (label, position) [U] and the labels in that order [U].
struct TdDesc {
  int32_t T, U, status, lab, ord;
  float w;
  int32_t pad[2];
};
static_assert(sizeof(TdDesc) == 32, "TdDesc is 8 words");

// Workspace of one utterance in floats from its base (every array on a 64-word boundary); C = T (U+1) grid cells.
struct TdLayout {
  size_t ma, ml, amb, lmb, zl, S, px, py, al, be, oy, ox, G, lp, words;
};
__host__ __device__ inline size_t td_up(size_t x) { return (x + 63) / 64 * 64; }
__host__ __device__ inline TdLayout td_layout(size_t T, size_t U) {
  TdLayout l;
  const size_t U1 = U + 1, C = T * U1;
  size_t o = 0;
  l.ma = o; o += td_up(T);            // f32 [T]        row maxima of am
  l.ml = o; o += td_up(U1);           // f32 [U+1]      row maxima of lm
  l.amb = o; o += td_up(T);           // f32 [T]        am[t, blank]
  l.lmb = o; o += td_up(U1);          // f32 [U+1]      lm[u, blank]
  l.zl = o; o += td_up(C);            // f32 [T][U+1]   am[t, l_{u+1}] + lm[u, l_{u+1}]  (column U unused)
  l.S = o; o += td_up(C);             // f32 [T][U+1]   the normaliser
  l.px = o; o += td_up(C);            // f32 [T][U+1]
  l.py = o; o += td_up(C);            // f32 [T][U+1]
  l.al = o; o += td_up(2 * C);        // f64 [T][U+1]   log alpha
  l.be = o; o += td_up(2 * C);        // f64 [T][U+1]   log beta
  l.oy = o; o += td_up(C);            // f32 [T][U+1]   occ_y
  l.ox = o; o += td_up(C);            // f32 [T][U+1]   occ_x
  l.G = o; o += td_up(C);             // f32 [T][U+1]   (occ_x + occ_y) / S
  l.lp = o; o += 64;                  // f64 log p, then i32 flag: a normaliser was 0, subnormal or non-finite
  l.words = o;
  return l;
}
__device__ inline size_t td_base(const TdDesc* desc, int n) {
  size_t o = 0;
  for (int m = 0; m < n; ++m) o += td_layout(desc[m].T, desc[m].U).words;
  return o;
}

}  // namespace pk2td
