// Persistent LSTM recurrence, one (sequence, direction) per XCD (gfx950, H = 512).
//
// The recurrences of different sequences do not depend on each other, so every (sequence, direction) pair is its own
// recurrence on its own XCD -- 4 sequences x 2 directions = the 8 XCDs of the part; more pairs queue up behind them:
//  * 32 workgroups (one per CU of the XCD; teams form by arrival order, pairs are handed out from a queue), workgroup r
//    owns hidden units 16r..16r+15, its 64 gate rows of W_hh (128 KB) stay in VGPRs;
//  * one batch row makes the recurrent product a matrix-VECTOR product: plain FMAs (the layout of the lanes is described
//    with the kernels below);
//  * h_t (2 KB) / the partial products (a 2 KB mailbox per workgroup) are exchanged through the XCD's own L2: plain stores
//    over a NaN sentinel, polled with L1-bypassing 16-byte loads, no flags.
// Tensors and their layouts are those of the step kernels (lstm.hip; y pre-filled with the sentinel, gates / cells kept for
// the backward pass), so the two implementations are interchangeable behind pk2_lstm_layer_fwd / _bwd.
// Replaces the same cuDNN RNN (reference models/lstm.py:49-58).
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>

#include "common.h"
#include "lstm_persist.h"
#include "persist_guard.h"

namespace pk2 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kSeqSentinel = 0x7fc0dead;
constexpr int kSH = 512;
constexpr int kSWgs = 32;                   // workgroups of a team = CUs of an XCD; 16 hidden units each
constexpr int kSeqTeams = 8;                // teams per XCD the control block has room for
constexpr int kSeqMaxTasks = 64;
constexpr long long kSeqSpinTicks = 1000LL * 1000 * 100;     // 1 s of the 100 MHz wall clock
// per team: [step % depth][reader][writer][16 units].  The hand-over stores are plain (XCD-local) ones, so the backward
// kernel walks all eight slots: a slot's reset by its reader then has seven steps and as many dependent exchanges to land
// before a writer stores to the slot again.
constexpr int kSeqMailDepth = 8;
constexpr int kSeqMailFloats = kSeqMailDepth * kSWgs * kSWgs * 16;

struct SeqCtl {
  unsigned arrive[8];
  unsigned next_task;
  unsigned abort;
  unsigned done;
  unsigned exited;        // workgroups that have left the kernel (round 6: the last one out runs the check)
  unsigned pad[4];
  struct Team { unsigned task[kSeqMaxTasks + 1]; unsigned bar; unsigned pad[62]; } team[8][kSeqTeams];
};

__device__ __forceinline__ unsigned seq_xcc_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 0x7;
}
__device__ __forceinline__ u32x4 seq_load16(const float* p) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// The hand-over stores: plain ones (see the notes on the kernels below).  (the s_nop: ">8-byte VMEM store data followed by
// a VALU write of the same VGPRs" hazard, invisible to the compiler inside an asm statement)
__device__ __forceinline__ void seq_store16(float* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void seq_store(float* p, float v) {
  asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ unsigned seq_load_u(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool seq_has_sentinel(u32x4 v) {
  return v.x == kSeqSentinel || v.y == kSeqSentinel || v.z == kSeqSentinel || v.w == kSeqSentinel;
}
__device__ __forceinline__ float seq_sig(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
__device__ __forceinline__ float seq_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.8853900817779268f * x)); }
template <int CTRL>
__device__ __forceinline__ float seq_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Workgroup barrier that waits for the LDS traffic only: __syncthreads() also waits for every outstanding global store
// and load of the thread (s_waitcnt vmcnt(0)), i.e. for the HBM traffic of the previous step.
__device__ __forceinline__ void seq_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// -DPK2_SEQ_PROFILE: phase timers of wave 0 of rank 0 of every team on its first pair (shader clock, s_memtime; the
// wall clock brackets the whole recurrence so that clocks convert to time), printed per team at the end of the pair.
#ifdef PK2_SEQ_PROFILE
#define SQ_NPH 8
#define SQ_T0() long long sq_acc_[SQ_NPH] = {0, 0, 0, 0, 0, 0, 0, 0}; long long sq_last_ = clock64(); const long long sq_w0_ = wall_clock64(); const long long sq_c0_ = sq_last_
#define SQ_T(k) do { const long long n_ = clock64(); sq_acc_[k] += n_ - sq_last_; sq_last_ = n_; } while (0)
#define SQ_PRINT(name, labels, steps) do { if (tid == 0 && rank == 0 && iter == 0) { const long long wt_ = wall_clock64() - sq_w0_, ct_ = clock64() - sq_c0_; \
    printf("%s xcd %d, %d steps, %.1f ns per step (wall), %.0f clocks per step; clocks per step %s: %lld | %lld | %lld | %lld | %lld | %lld | %lld | %lld\n", name, s_i[2], steps, \
           10.0 * (double)wt_ / (steps), (double)ct_ / (steps), labels, sq_acc_[0] / (steps), sq_acc_[1] / (steps), sq_acc_[2] / (steps), sq_acc_[3] / (steps), sq_acc_[4] / (steps), \
           sq_acc_[5] / (steps), sq_acc_[6] / (steps), sq_acc_[7] / (steps)); } } while (0)
#else
#define SQ_T0() do { } while (0)
#define SQ_T(k) do { } while (0)
#define SQ_PRINT(name, labels, steps) do { } while (0)
#endif

// A poll that keeps failing reads the wall clock every 256 rounds; after 1 s (or when somebody else gave up) it raises
// the abort flag.
struct SeqSpin {
  SeqCtl* ctl; long long t0; unsigned n; long long limit;
  __device__ __forceinline__ explicit SeqSpin(SeqCtl* c) : ctl(c), t0(0), n(0), limit(kSeqSpinTicks) {}
  __device__ __forceinline__ bool expired() {
    if ((++n & 255u) != 0u) return false;
    const long long now = wall_clock64();
    if (t0 == 0) t0 = now;
    if (now - t0 > limit || seq_load_u(&ctl->abort)) {
      __hip_atomic_store(&ctl->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return true;
    }
    return false;
  }
};

// Team formation and the queue of (sequence, direction) pairs, shared by both kernels.
struct SeqRole { int rank; SeqCtl::Team* team; int team_index; };
__device__ __forceinline__ bool seq_register(SeqCtl* ctl, int* s_i, SeqRole* role) {
  if (threadIdx.x == 0) {
    const unsigned xcd = seq_xcc_id();
    const unsigned slot = __hip_atomic_fetch_add(&ctl->arrive[xcd], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_i[0] = (int)(slot % kSWgs); s_i[1] = (int)(slot / kSWgs); s_i[2] = (int)xcd; s_i[3] = 0;
  }
  __syncthreads();
  if (s_i[1] >= kSeqTeams) return false;
  role->rank = s_i[0];
  role->team = &ctl->team[s_i[2]][s_i[1]];
  role->team_index = s_i[1] * 8 + s_i[2];       // (team-major: the teams a launch uses are the first 8 * teams mailboxes)
  return true;
}
// Next pair of this team (-1: none left / abort).  s_i[3] = abort flag of the workgroup, s_i[4] = the task.
__device__ __forceinline__ int seq_next_task(SeqCtl* ctl, const SeqRole& role, int iter, int ntasks, int* s_i) {
  if (threadIdx.x == 0) {
    unsigned k;
    if (role.rank == 0) {
      k = __hip_atomic_fetch_add(&ctl->next_task, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&role.team->task[iter], k + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      SeqSpin spin(ctl);
      unsigned k1;
      while ((k1 = seq_load_u(&role.team->task[iter])) == 0u) {
        if (spin.expired()) { s_i[3] = 1; k1 = 1u << 30; break; }
      }
      k = k1 - 1u;
    }
    s_i[4] = (int)k;
  }
  __syncthreads();
  const int k = s_i[4];
  return (s_i[3] || k >= ntasks) ? -1 : k;
}
__device__ __forceinline__ bool seq_team_barrier(SeqCtl* ctl, const SeqRole& role, unsigned* nbar, int* s_i) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned target = (unsigned)kSWgs * ++*nbar;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(&role.team->bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SeqSpin spin(ctl);
    while (seq_load_u(&role.team->bar) < target) {
      if (spin.expired()) { s_i[3] = 1; break; }
    }
  }
  __syncthreads();
  return s_i[3] == 0;
}

struct SeqFwdParams {
  const float* gx;    // [T][B][D*4H]
  const float* whh;   // [D][4H][H]
  const float* bhh;   // [D][4H] or null
  float* y;           // [T][B][D*H], pre-filled with the sentinel
  float* gates;       // [D][T][B][4H]
  float* cells;       // [D][T][B][H]
  int B, T, D;
};

struct SeqBwdParams {
  const float* dy;     // [T][B][D*H]
  const float* whh;    // [D][4H][H]
  const float* gates;  // [D][T][B][4H]
  const float* cells;  // [D][T][B][H]
  float* dgx;          // [T][B][D*4H]
  float* mail;         // [teams][kSeqMailDepth][32 readers][32 writers][16 units], all sentinel
  int B, T, D;
  float* dbias_ih;     // [D][4H] += sum over frames and sequences of d gx (null: not wanted), likewise dbias_hh
  float* dbias_hh;
};

// The recurrent weight gradient from inside the backward recurrence (lstm_bwd_seq2_wgrad).  Kept out of
// SeqBwdParams so that the kernel arguments -- and with them the code -- of lstm_bwd_seq2 stay what they were.
struct SeqWgradParams {
  const float* y;      // [T][B][D*H], the forward pass's output (complete, read-only)
  float* ws;           // [B*D][4H][H]: the slice of dW_hh[d] every (sequence, direction) pair has summed over its frames
};

// ---- The kernels (round 4: lstm_fwd_seq2 / lstm_bwd_seq2), the step's critical path cut down ---------------------------
// What the phase timers (-DPK2_SEQ_PROFILE, profiles/r04_seq_phases.txt) charged a step of the round-2 kernels (since
// retired) besides the round trip through L2, and what changed (forward 1.47 -> 0.97 us, backward 1.79 -> 1.14
// us per step, T = 589, B = 4):
//  * The hand-over stores were agent-scope (sc1) stores.  On this multi-XCD part an agent-scope store is written THROUGH
//    the XCD's L2 to the fabric; a team lives on one XCD, whose L2 is the coherence point of its 32 CUs, so plain stores
//    (which the write-through vector L1 forwards to L2, and which vmcnt acknowledges there) are enough as long as the
//    readers poll with L1-bypassing loads: backward 1.95 -> 1.22 us per step by that alone (its 2 KB of scattered partial
//    sums per workgroup and step), forward 1.09 -> 0.98.  The data is
//    polled on itself over a sentinel, so no ordering between stores is assumed; the backward mailboxes are a ring of
//    eight step slots, so that a slot's reset has seven steps to land before the slot is written again.
//  * `s_waitcnt vmcnt(0)` counts the WAVE's operations, not the lane's: a poll waits for every vector-memory operation the
//    wave has in flight.  Forward: waves 0, 1 poll (a granule per lane) and have nothing else in flight but their h
//    stores; wave 2 prefetches the input projections of the whole workgroup two steps ahead into an LDS ring, wave 3
//    writes gate activations and cells (handed over in LDS) to HBM a step later -- both behind their h stores.
//    Backward: wave 0 polls; wave 1 prefetches the forward pass's values, turns them into the per-unit factors of the
//    gate derivatives (everything that does not depend on the incoming d h, tanh(c) included) two steps ahead in LDS,
//    and writes d gx out -- behind its share of the partial sums.  (Scalar loads for the prefetch were tried first:
//    slower, the scalar cache misses queue up behind each other and the LDS waits share their counter.)
//  * What the compiler does to a persistent loop: it waits for a load where the VALUE is first needed, so (i) the waits
//    for W_hh landed inside the step loop (an `s_waitcnt vmcnt(0)` in every product, which then waits for the step's own
//    stores and prefetches: explicit wait before the loop), (ii) a load under a branch is waited for at the join, i.e. at
//    once (unconditional loads from clamped pointers), (iii) a register rotation copies the values just requested (no
//    rotation: one set of registers in flight for a whole step).  Addresses walk pointers (the per-step 64-bit index
//    arithmetic was 150-300 clocks of a 2300-clock step: a lone wave issues an instruction every ~5 clocks).
//  * Forward product: a lane owns a 32-k slice of the FOUR gate rows of one unit (was: 128 k's of one row): 8
//    ds_read_b128 instead of 32 per lane and step, all in flight before the first FMA, packed FMAs in eight independent
//    chains (tools/ubench/valu_rate.hip: 5.1 clocks per v_pk_fma_f32 in independent chains, 8.4 in one chain); the 16
//    slices of a unit are the 16 lanes of a DPP row, added by a 4-level butterfly (v_add_f32_dpp in inline asm: left to
//    the compiler the four chains become v_pk_add_f32 with two v_mov_dpp each); lane j of the row applies gate j's
//    nonlinearity (tanh as a scaled sigmoid: one exp2 + one rcp for all four gates at once), lane 0 collects them.
//  * Backward: ONE wave gathers the mailbox (two 16-byte granules per lane: writers j and j + 16, a DPP row per group
//    of 4 units), adds the 32 partials with the same butterfly and finishes the gate derivatives in the same lanes: no
//    LDS round trip and no barrier between the poll and the pointwise work, no 32-deep serial sum on 16 threads.  A lane
//    PAIR owns a 16-byte granule of the partial d h (4 columns x half of the rows each), so the partials leave as one
//    16-byte store per pair instead of two scattered 4-byte stores per lane; the reader resets a slot behind its own
//    partials (issuing the two reset stores takes ~300 clocks).
//  * Tried and dropped: two polls in flight half a round trip apart (the arrival is noticed with half the granularity, the
//    polling traffic doubles): forward 1.02 -> 1.04 us per step; s_sleep before the first poll or between polls: slower
//    with plain stores (it paid only while the stores were agent-scope ones: backward 1.99 -> 1.56 us at 16 x 64 clocks,
//    i.e. polling a line that is being written through costs the writer).
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define PK2_CONSTANT_AS __attribute__((address_space(4)))

// Butterfly sum over the 16 lanes of a DPP row; every lane of the row ends with the same bits (each level adds a pair of
// values that both partners hold, and float addition is commutative).
__device__ __forceinline__ float seq_row_sum(float v) {
  v += seq_dpp<0xB1>(v);         // quad_perm [1,0,3,2]
  v += seq_dpp<0x4E>(v);         // quad_perm [2,3,0,1]
  v += seq_dpp<0x141>(v);        // row_half_mirror: the other quad of the half row (quads are uniform by now)
  v += seq_dpp<0x140>(v);        // row_mirror: the other half row
  return v;
}
// Four of them at once, level by level (left to the compiler the four chains are paired into v_pk_add_f32, which has no
// DPP form: two v_mov_dpp + a packed add per level and pair -- three times the instructions).  A DPP operand written by
// the previous VALU instruction needs two wait states: the s_nop covers the first level, the other three chains the rest.
__device__ __forceinline__ void seq_row_sum4(float& a, float& b, float& c, float& d) {
#define PK2_SEQ_DPP_LEVEL(ctrl)                                              \
  "v_add_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf\n\t"         \
  "v_add_f32_dpp %1, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf\n\t"         \
  "v_add_f32_dpp %2, %2, %2 " ctrl " row_mask:0xf bank_mask:0xf\n\t"         \
  "v_add_f32_dpp %3, %3, %3 " ctrl " row_mask:0xf bank_mask:0xf\n\t"
  asm volatile("s_nop 1\n\t" PK2_SEQ_DPP_LEVEL("quad_perm:[1,0,3,2]") PK2_SEQ_DPP_LEVEL("quad_perm:[2,3,0,1]")
               PK2_SEQ_DPP_LEVEL("row_half_mirror") PK2_SEQ_DPP_LEVEL("row_mirror")
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef PK2_SEQ_DPP_LEVEL
}
__device__ __forceinline__ const float* seq_uniform_ptr(const float* ptr) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(ptr);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}
// 16 contiguous bytes through the scalar cache (the address must be wave-uniform and 16-byte aligned).
__device__ __forceinline__ f32x4 seq_sload16(const float* ptr) {
  return *reinterpret_cast<const PK2_CONSTANT_AS f32x4*>(reinterpret_cast<unsigned long long>(ptr));
}
template <int LANE>
__device__ __forceinline__ float seq_writelane(float v, float old) {        // old with lane LANE replaced by the (uniform) v
  asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(v), "n"(LANE));
  return old;
}

__device__ __forceinline__ void lstm_fwd_seq2_body(const SeqFwdParams& p, SeqCtl* ctl) {
  constexpr int H = kSH;
  constexpr int kSlicePitch = 36;           // 32 + 4: the 16 slices a lane group reads side by side start on 16 different bank quads
  __shared__ __attribute__((aligned(16))) float hs[2][16 * kSlicePitch];
  __shared__ float gxs[3][64];              // input projections [step % 3][gate * 16 + unit], written two steps ahead by wave 2
  __shared__ float outs[2][80];             // [step & 1]: gate activations [gate * 16 + unit], cells [64 + unit]; wave 3 writes them out
  __shared__ int s_i[8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  SeqRole role;
  if (!seq_register(ctl, s_i, &role)) return;
  const int rank = role.rank, B = p.B, T = p.T, D = p.D;
  // lane roles: a 16-lane DPP row = one hidden unit, lane % 16 = its k-slice; lane j < 4 of the row finishes gate j
  const int ul = lane >> 4, l16 = lane & 15;
  const int uw = 4 * w + ul;                             // unit within the workgroup
  const int gu = 16 * rank + uw;
  const bool unit_lane = l16 == 0, gate_lane = l16 < 4;
  const bool poller = w < 2;                             // waves 0, 1 poll (a granule per lane); waves 2, 3 do the HBM traffic
  const int gran = w * 64 + lane;                        // granule of h this lane polls (128 per step)
  // gate j's nonlinearity as a * rcp(1 + exp2(s * x)) + b: sigmoid (1, -log2 e, 0), tanh (2, -2 log2 e, -1)
  const float act_s = l16 == 2 ? -2.8853900817779268f : -1.4426950408889634f;
  const float act_a = l16 == 2 ? 2.0f : 1.0f, act_b = l16 == 2 ? -1.0f : 0.0f;
  const int pre_idx = 16 * (l16 & 3) + uw, out_idx = gate_lane ? 16 * l16 + uw : 0;
  const size_t yrow = (size_t)D * H;
  unsigned nbar = 0;
  for (int iter = 0; iter <= kSeqMaxTasks; ++iter) {
    const int task = seq_next_task(ctl, role, iter, B * D, s_i);
    if (task < 0) return;
    const int b = task / D, d = task % D;
    f32x2 wa[4][16];                                     // W_hh[d][g*H + gu][32 l16 + 2 i, + 1]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float* wrow = p.whh + ((size_t)d * 4 * H + (size_t)g * H + gu) * H + 32 * l16;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + i * 4);
        wa[g][2 * i] = f32x2{v[0], v[1]};
        wa[g][2 * i + 1] = f32x2{v[2], v[3]};
      }
    }
    const float bias = (gate_lane && p.bhh) ? p.bhh[(size_t)d * 4 * H + (size_t)l16 * H + gu] : 0.f;
    // Everything addressed by time walks a pointer: t = step (d = 0) or T - 1 - step (d = 1).
    const ptrdiff_t tdir = d == 0 ? 1 : -1;
    const size_t t0 = d == 0 ? 0 : (size_t)(T - 1);
    const ptrdiff_t y_stride = tdir * (ptrdiff_t)((size_t)B * yrow);
    float* y_out = p.y + (t0 * B + b) * yrow + (size_t)d * H + gu;                        // h_t of the lane's unit
    const float* y_poll = p.y + (t0 * B + b) * yrow + (size_t)d * H + 4 * gran - y_stride;  // the granule of h_{t-1}
    // wave 2: lane = gate * 16 + unit of the workgroup's input projections; wave 3: the same lanes store the activations,
    // its lanes 0..15 the cells
    const ptrdiff_t gx_stride = tdir * (ptrdiff_t)((size_t)B * D * 4 * H);
    const float* gx_in = p.gx + (t0 * B + b) * ((size_t)D * 4 * H) + (size_t)d * 4 * H + (size_t)(lane >> 4) * H + 16 * rank + (lane & 15);
    const ptrdiff_t gates_stride = tdir * (ptrdiff_t)((size_t)B * 4 * H), cells_stride = tdir * (ptrdiff_t)((size_t)B * H);
    float* gates_out = p.gates + (((size_t)d * T + t0) * B + b) * 4 * H + (size_t)(lane >> 4) * H + 16 * rank + (lane & 15);
    float* cells_out = p.cells + (((size_t)d * T + t0) * B + b) * H + 16 * rank + (lane & 15);
    // (loads are unconditional and walk a clamped pointer: a load under a branch makes the compiler wait for it at the
    // join, i.e. at once)
    float gnext = 0.f;
    if (w == 2) {
      gxs[0][lane] = gx_in[0];
      gx_in += T > 1 ? gx_stride : 0;
      gxs[1][lane] = gx_in[0];
      gx_in += T > 2 ? gx_stride : 0;
      gnext = gx_in[0];
      gx_in += T > 3 ? gx_stride : 0;
    }
    // W_hh, bias and the first input projections have arrived BEFORE the loop: left to itself the compiler waits for them
    // at their first use, inside the loop -- an s_waitcnt vmcnt(0) in every step's product, which then also waits for the
    // step's own stores and prefetches.
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
    __syncthreads();
    float cstate = 0.f;
    bool timed_out = false;
    SeqSpin spin(ctl);
    spin.limit = 10 * kSeqSpinTicks;      // until the first exchange has worked: a team mate dispatched late is not a deadlock
    SQ_T0();
    for (int step = 0; step < T; ++step) {
      if (step == 2) { spin.limit = kSeqSpinTicks; spin.t0 = 0; }
      const int buf = step & 1;
      const float pre = gxs[step % 3][pre_idx] + bias;
      // ---- gather h_{t-1} of this (sequence, direction): 512 floats = 128 granules of 16 bytes -----------------------
      if (step > 0 && poller) {
        u32x4 v = seq_load16(y_poll);
        while (seq_has_sentinel(v)) {
          if (spin.expired()) { timed_out = true; break; }
          v = seq_load16(y_poll);
        }
        *reinterpret_cast<u32x4*>(&hs[buf][(gran >> 3) * kSlicePitch + 4 * (gran & 7)]) = v;
      }
      y_poll += y_stride;
      SQ_T(0);
      if (timed_out) s_i[3] = 1;
      seq_lds_barrier();
      SQ_T(1);
      if (s_i[3]) return;
      // ---- recurrent product: the lane's 32-k slice of the unit's four gate rows ---------------------------------------
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      if (step > 0) {
        const float* hq = &hs[buf][l16 * kSlicePitch];
        f32x2 a0 = {0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0, c0 = a0, c1 = a0, c2 = a0, c3 = a0;
        f32x4 hva[8];                                     // all eight reads in flight before the first FMA
#pragma unroll
        for (int i = 0; i < 8; ++i) hva[i] = *reinterpret_cast<const f32x4*>(hq + 4 * i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const f32x4 hv = hva[i];
          const f32x2 h01 = {hv[0], hv[1]}, h23 = {hv[2], hv[3]};
          a0 = __builtin_elementwise_fma(wa[0][2 * i], h01, a0); c0 = __builtin_elementwise_fma(wa[0][2 * i + 1], h23, c0);
          a1 = __builtin_elementwise_fma(wa[1][2 * i], h01, a1); c1 = __builtin_elementwise_fma(wa[1][2 * i + 1], h23, c1);
          a2 = __builtin_elementwise_fma(wa[2][2 * i], h01, a2); c2 = __builtin_elementwise_fma(wa[2][2 * i + 1], h23, c2);
          a3 = __builtin_elementwise_fma(wa[3][2 * i], h01, a3); c3 = __builtin_elementwise_fma(wa[3][2 * i + 1], h23, c3);
        }
        s0 = (a0[0] + a0[1]) + (c0[0] + c0[1]);
        s1 = (a1[0] + a1[1]) + (c1[0] + c1[1]);
        s2 = (a2[0] + a2[1]) + (c2[0] + c2[1]);
        s3 = (a3[0] + a3[1]) + (c3[0] + c3[1]);
        seq_row_sum4(s0, s1, s2, s3);
      }
#ifdef PK2_SEQ_PROFILE
      asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3));
#endif
      SQ_T(2);
      // ---- gates: lane j of the row takes gate j --------------------------------------------------------------------------
      const float x = pre + (l16 == 0 ? s0 : l16 == 1 ? s1 : l16 == 2 ? s2 : s3);
      const float act = fmaf(act_a, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(act_s * x)), act_b);
      const float fg = seq_dpp<0x101>(act), gg = seq_dpp<0x102>(act), og = seq_dpp<0x103>(act);     // row_shl 1, 2, 3
      cstate = fg * cstate + act * gg;                    // (meaningful in the row's lane 0 only)
      const float h = og * seq_tanh(cstate);
      if (unit_lane) seq_store(y_out, h);
      y_out += y_stride;
      SQ_T(3);
      // ---- behind the hand-over: what the backward pass needs goes to HBM through wave 3, the input projections of the
      // step after next come in through wave 2 (the polling waves keep no other vector-memory operation in flight) ---------
      if (gate_lane) outs[buf][out_idx] = act;
      if (unit_lane) outs[buf][64 + uw] = cstate;
      if (w == 2) {
        gxs[(step + 2) % 3][lane] = gnext;                // (loaded a step ago)
        gnext = *gx_in;                                   // step + 3 (clamped to the last step)
        gx_in += step + 4 < T ? gx_stride : 0;
      }
      if (w == 3 && step > 0) {                           // the previous step's values (a barrier lies between)
        *gates_out = outs[buf ^ 1][lane];
        if (lane < 16) *cells_out = outs[buf ^ 1][64 + lane];
        gates_out += gates_stride; cells_out += cells_stride;
      }
      SQ_T(4);
    }
    __syncthreads();
    if (w == 3) {
      *gates_out = outs[(T - 1) & 1][lane];
      if (lane < 16) *cells_out = outs[(T - 1) & 1][64 + lane];
    }
    SQ_PRINT("lstm_fwd_seq2", "(poll | lds + barrier | product + row sums | gates + h store | lds hand-over, wave 2 / 3 traffic)", T);
    if (tid == 0 && rank == 0) __hip_atomic_fetch_add(&ctl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!seq_team_barrier(ctl, role, &nbar, s_i)) return;
  }
}

// XPROJ (lstm_fwd_seq2_xproj): the recurrence computes its own input projections gx = inp W_ih^T + b_ih on the MFMA pipe,
// which lstm_fwd_seq2 leaves idle for the whole launch.  The workgroup has eight waves: waves 0..3 run the recurrence of
// lstm_fwd_seq2 (minus wave 2's prefetch of gx), waves 4..7 -- one more per SIMD -- are projection waves and run a block of
// 32 time steps ahead of them:
//  * projection wave g owns gate g's 16 rows of the workgroup's 64 (all of K: no partial sums to add, the k order of a
//    result is fixed) and both 16-step halves of a block: G[16 rows][2 x 16 steps] in accumulators of
//    v_mfma_f32_16x16x4_f32 (the f32 fmaf chain), two per half -- the k's with the same k % 2 form one chain of K / 2
//    products, the two are added at the end of the block (four per half do not fit 256 registers) -- which take turns (40 clocks of dependent latency, 32 of issue);
//  * a loop iteration = one step of the recurrence = one chunk of 32 k's: 16 MFMAs per wave (512 clocks of a ~2100-clock
//    step), so a block of 32 steps covers K = 1024 (in_size 80: three chunks, the rest of the block idles);
//  * its rows of W_ih (16 x K): the first 16 chunks in registers (128 per lane), the other 16 in LDS (4 x 32 KB, lane-major
//    16-byte granules: conflict-free), read once per block;
//  * the chunk of inp (32 steps x 32 k's = 4 KB, a 16-byte granule per projection thread, clamped to the last step) is
//    loaded two iterations ahead and staged in LDS a barrier ahead, so the 32 CUs of a team read inp once from their L2;
//  * the projection waves take part in the step's one s_barrier and in nothing else of the recurrence; the finished
//    block (+ b_ih) goes into an LDS ring of two blocks, from which the recurrence waves read their step's 64 values as
//    they read gxs in lstm_fwd_seq2 -- behind the step's barrier, not in front of it: block n is written in the iteration
//    of step 32 n - 1, so that barrier lies between the write and step 32 n's read, and 32 barriers between the last read
//    of block n - 2 and the write;
//  * before step 0 the recurrence waves sit out 32 barriers while block 0 is computed;
//  * the f32 MFMA runs at the vector rate on the SIMD a projection wave shares with a recurrence wave, so the chunk is
//    issued while that wave polls, not while it multiplies: the projection waves rest behind the barrier (kXSleep) and
//    the recurrence waves run at a higher priority (the measurements).
struct SeqXprojParams {
  const float* inp;   // [T][B][K]
  const float* wih;   // [D][4H][K]
  const float* bih;   // [D][4H] or null
  int K;              // in_size: 80 or 1024, the kernel's template argument
};
constexpr int kXBlock = 32;                 // time steps per block = k's per chunk = iterations the projection waves run ahead
constexpr int kXPitch = 36;                 // (as kSlicePitch)
#ifndef PK2_SEQ_XSLEEP
#define PK2_SEQ_XSLEEP 17
#endif
constexpr int kXSleep = PK2_SEQ_XSLEEP;     // x 64 clocks: the projection waves' rest behind a step's barrier (experiment builds: -DPK2_SEQ_XSLEEP=n)

template <int K>
__device__ __forceinline__ void lstm_fwd_seq2_xproj_body(const SeqFwdParams& p, const SeqXprojParams& xp, SeqCtl* ctl) {
  constexpr int H = kSH;
  constexpr int kSlicePitch = 36;
  constexpr int NCH = (K + 31) / 32;                                    // chunks of 32 k's (the last one may be short)
  constexpr int NREG = NCH < 16 ? NCH : 16, NLDS = NCH - NREG;          // chunks of W_ih in registers / in LDS
  static_assert(K % 4 == 0 && NCH >= 1 && NCH <= kXBlock, "a block of 32 iterations holds at most 32 chunks of 16-byte granules");
  __shared__ __attribute__((aligned(16))) float hs[2][16 * kSlicePitch];
  __shared__ __attribute__((aligned(16))) float xring[2][kXBlock][64];  // input projections [block & 1][step % 32][gate * 16 + unit]
  __shared__ __attribute__((aligned(16))) float xs[2][kXBlock][kXPitch];  // the chunk of inp [iteration & 1][step % 32][k % 32]
  __shared__ __attribute__((aligned(16))) float wl[NLDS > 0 ? NLDS : 1][2][256][4];  // W_ih [chunk - NREG][half][projection thread]
  __shared__ float outs[2][80];
  __shared__ int s_i[8];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  SeqRole role;
  if (!seq_register(ctl, s_i, &role)) return;
  const int rank = role.rank, B = p.B, T = p.T, D = p.D;
  const int ul = lane >> 4, l16 = lane & 15;
  const int uw = 4 * (w & 3) + ul;
  const int gu = 16 * rank + uw;
  const bool unit_lane = l16 == 0, gate_lane = l16 < 4;
  const bool poller = w < 2;
  const int gran = (w & 1) * 64 + lane;
  const float act_s = l16 == 2 ? -2.8853900817779268f : -1.4426950408889634f;
  const float act_a = l16 == 2 ? 2.0f : 1.0f, act_b = l16 == 2 ? -1.0f : 0.0f;
  const int pre_idx = 16 * (l16 & 3) + uw, out_idx = gate_lane ? 16 * l16 + uw : 0;
  const size_t yrow = (size_t)D * H;
  unsigned nbar = 0;
  for (int iter = 0; iter <= kSeqMaxTasks; ++iter) {
    const int task = seq_next_task(ctl, role, iter, B * D, s_i);
    if (task < 0) return;
    const int b = task / D, d = task % D;
    if (w >= 4) {
      // ---- projection waves ------------------------------------------------------------------------------------------------
      // MFMA operands: lane = (m = lane % 16, kq = lane / 16); instruction e of a chunk multiplies the k's 32 c + 8 kq + e:
      // A = W_ih[row m][k], B = inp[step n = m][k]; D: lane holds rows 4 kq .. 4 kq + 3 of column (step) m.
      const int q = tid - 256, pw = w - 4, m = l16, kq = ul;
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 wreg[NREG][2];
      {
        const float* wrow = xp.wih + ((size_t)d * 4 * H + (size_t)pw * H + 16 * rank + m) * K;
        auto wload = [&](int c, int h) -> f32x4 {          // (K is a multiple of 4: a granule lies inside the row or outside)
          const int k = 32 * c + 8 * kq + 4 * h;
          const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + (k < K ? k : 0));
          return k < K ? v : zero4;
        };
#pragma unroll 2
        for (int c = NREG; c < NCH; ++c) {                 // (first, a few at a time: the registers are for the chunks that stay)
          *reinterpret_cast<f32x4*>(&wl[c - NREG][0][q][0]) = wload(c, 0);
          *reinterpret_cast<f32x4*>(&wl[c - NREG][1][q][0]) = wload(c, 1);
        }
#pragma unroll
        for (int c = 0; c < NREG; ++c) { wreg[c][0] = wload(c, 0); wreg[c][1] = wload(c, 1); }
      }
      f32x4 bi = zero4;
      if (xp.bih) bi = *reinterpret_cast<const f32x4*>(xp.bih + (size_t)d * 4 * H + (size_t)pw * H + 16 * rank + 4 * kq);
      // the thread's 16-byte granule of chunk c of a block: step 32 block + tq (clamped: the last block), k's 32 c + 4 k4 ..;
      // loads are unconditional (see lstm_fwd_seq2), granules past K read the row's start and count 0
      const int tq = q >> 3, k4 = q & 7;
      auto xrow = [&](int block) -> const float* {
        const int s = min(kXBlock * block + tq, T - 1);
        const size_t t = d == 0 ? (size_t)s : (size_t)(T - 1 - s);
        return xp.inp + (t * B + b) * (size_t)K;
      };
      auto xload = [&](const float* row, int c) -> f32x4 {
        const int k = 32 * c + 4 * k4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (k < K ? k : 0));
        return k < K ? v : zero4;
      };
      const float* xrow_cur = xrow(0);
      const float* xrow_next = xrow(1);
      f32x4 xnext = xload(xrow_cur, 0);
      *reinterpret_cast<f32x4*>(&xs[0][tq][4 * k4]) = xnext;
      xnext = NCH > 1 ? xload(xrow_cur, 1) : zero4;
      f32x4 acc0[2] = {zero4, zero4}, acc1[2] = {zero4, zero4};     // [k % 2]: chains of K / 2 products
      __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): as below
      __syncthreads();
#ifdef PK2_SEQ_PROFILE
      long long xq_bar = 0, xq_work = 0;
#endif
      const int iters = T + kXBlock;
      for (int i0 = 0; i0 < iters; i0 += kXBlock) {
        if (i0 > 0) { xrow_cur = xrow_next; xrow_next = xrow((i0 >> 5) + 1); }
#pragma unroll
        for (int c = 0; c < kXBlock; ++c) {
          const int i = i0 + c;
          if (i >= iters) break;
#ifdef PK2_SEQ_PROFILE
          const long long xq0 = clock64();
#endif
          seq_lds_barrier();
          if (s_i[3]) return;
#ifdef PK2_SEQ_PROFILE
          const long long xq1 = clock64();
          xq_bar += xq1 - xq0;
#endif
          // The f32 MFMAs run at the VALU's rate on the SIMD they share with a recurrence wave: issued right behind the
          // barrier they delay that wave's product by their whole length (measured: product + row sums 806 -> 1331 clocks).
          // So the chunk waits until the recurrence waves have stored h and only poll (~930 clocks behind the barrier;
          // not while block 0 is computed, when they only sit at the barrier).
          if (i0 > 0) __builtin_amdgcn_s_sleep(kXSleep);
          // the next iteration's chunk of inp into LDS (loaded an iteration ago), the one after it requested
          if ((c + 1) % kXBlock < NCH) *reinterpret_cast<f32x4*>(&xs[(c + 1) & 1][tq][4 * k4]) = xnext;
          if ((c + 2) % kXBlock < NCH) xnext = xload(c + 2 < kXBlock ? xrow_cur : xrow_next, (c + 2) % kXBlock);
          if (c < NCH) {
            f32x4 a0, a1;
            if (c < NREG) { a0 = wreg[c < NREG ? c : 0][0]; a1 = wreg[c < NREG ? c : 0][1]; }
            else {
              a0 = *reinterpret_cast<const f32x4*>(&wl[c < NREG ? 0 : c - NREG][0][q][0]);
              a1 = *reinterpret_cast<const f32x4*>(&wl[c < NREG ? 0 : c - NREG][1][q][0]);
            }
            const float* x0 = &xs[c & 1][m][8 * kq];
            const float* x1 = &xs[c & 1][16 + m][8 * kq];
            const f32x4 b00 = *reinterpret_cast<const f32x4*>(x0), b01 = *reinterpret_cast<const f32x4*>(x0 + 4);
            const f32x4 b10 = *reinterpret_cast<const f32x4*>(x1), b11 = *reinterpret_cast<const f32x4*>(x1 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc0[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b00[e], acc0[e & 1], 0, 0, 0);
              acc1[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b10[e], acc1[e & 1], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc0[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b01[e], acc0[e & 1], 0, 0, 0);
              acc1[e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b11[e], acc1[e & 1], 0, 0, 0);
            }
          }
          if (c == kXBlock - 1) {          // the block is complete: into the ring, a barrier ahead of its first reader
            float (*ring)[64] = xring[(i >> 5) & 1];
            *reinterpret_cast<f32x4*>(&ring[m][16 * pw + 4 * kq]) = (acc0[0] + acc0[1]) + bi;
            *reinterpret_cast<f32x4*>(&ring[16 + m][16 * pw + 4 * kq]) = (acc1[0] + acc1[1]) + bi;
#pragma unroll
            for (int e = 0; e < 2; ++e) { acc0[e] = zero4; acc1[e] = zero4; }
          }
#ifdef PK2_SEQ_PROFILE
          xq_work += clock64() - xq1;
#endif
        }
      }
#ifdef PK2_SEQ_PROFILE
      if (q == 0 && rank == 0 && iter == 0)
        printf("lstm_fwd_seq2_xproj<%d> projection wave 4, %d iterations: %lld clocks per iteration at the barrier | %lld on its chunk\n", K, iters,
               xq_bar / iters, xq_work / iters);
#endif
      __syncthreads();
    } else {
      // ---- recurrence waves: lstm_fwd_seq2 with the input projections from the ring ------------------------------------------
      // (they win the issue arbitration of their SIMD against its projection wave: a poll's compare does not queue behind MFMAs)
      __builtin_amdgcn_s_setprio(3);
      f32x2 wa[4][16];                                     // W_hh[d][g*H + gu][32 l16 + 2 i, + 1]
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float* wrow = p.whh + ((size_t)d * 4 * H + (size_t)g * H + gu) * H + 32 * l16;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + i * 4);
          wa[g][2 * i] = f32x2{v[0], v[1]};
          wa[g][2 * i + 1] = f32x2{v[2], v[3]};
        }
      }
      const float bias = (gate_lane && p.bhh) ? p.bhh[(size_t)d * 4 * H + (size_t)l16 * H + gu] : 0.f;
      const ptrdiff_t tdir = d == 0 ? 1 : -1;
      const size_t t0 = d == 0 ? 0 : (size_t)(T - 1);
      const ptrdiff_t y_stride = tdir * (ptrdiff_t)((size_t)B * yrow);
      float* y_out = p.y + (t0 * B + b) * yrow + (size_t)d * H + gu;
      const float* y_poll = p.y + (t0 * B + b) * yrow + (size_t)d * H + 4 * gran - y_stride;
      const ptrdiff_t gates_stride = tdir * (ptrdiff_t)((size_t)B * 4 * H), cells_stride = tdir * (ptrdiff_t)((size_t)B * H);
      float* gates_out = p.gates + (((size_t)d * T + t0) * B + b) * 4 * H + (size_t)(lane >> 4) * H + 16 * rank + (lane & 15);
      float* cells_out = p.cells + (((size_t)d * T + t0) * B + b) * H + 16 * rank + (lane & 15);
      __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): W_hh is there before the loop (see lstm_fwd_seq2)
      __syncthreads();
      for (int i = 0; i < kXBlock; ++i) {      // block 0 of the projections
        seq_lds_barrier();
        if (s_i[3]) return;
      }
      float cstate = 0.f;
      bool timed_out = false;
      SeqSpin spin(ctl);
      spin.limit = 10 * kSeqSpinTicks;
      SQ_T0();
      for (int step = 0; step < T; ++step) {
        if (step == 2) { spin.limit = kSeqSpinTicks; spin.t0 = 0; }
        const int buf = step & 1;
        if (step > 0 && poller) {
          u32x4 v = seq_load16(y_poll);
          while (seq_has_sentinel(v)) {
            if (spin.expired()) { timed_out = true; break; }
            v = seq_load16(y_poll);
          }
          *reinterpret_cast<u32x4*>(&hs[buf][(gran >> 3) * kSlicePitch + 4 * (gran & 7)]) = v;
        }
        y_poll += y_stride;
        SQ_T(0);
        if (timed_out) s_i[3] = 1;
        seq_lds_barrier();
        SQ_T(1);
        if (s_i[3]) return;
        const float pre = xring[(step >> 5) & 1][step & 31][pre_idx] + bias;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (step > 0) {
          const float* hq = &hs[buf][l16 * kSlicePitch];
          f32x2 a0 = {0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0, c0 = a0, c1 = a0, c2 = a0, c3 = a0;
          f32x4 hva[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) hva[i] = *reinterpret_cast<const f32x4*>(hq + 4 * i);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const f32x4 hv = hva[i];
            const f32x2 h01 = {hv[0], hv[1]}, h23 = {hv[2], hv[3]};
            a0 = __builtin_elementwise_fma(wa[0][2 * i], h01, a0); c0 = __builtin_elementwise_fma(wa[0][2 * i + 1], h23, c0);
            a1 = __builtin_elementwise_fma(wa[1][2 * i], h01, a1); c1 = __builtin_elementwise_fma(wa[1][2 * i + 1], h23, c1);
            a2 = __builtin_elementwise_fma(wa[2][2 * i], h01, a2); c2 = __builtin_elementwise_fma(wa[2][2 * i + 1], h23, c2);
            a3 = __builtin_elementwise_fma(wa[3][2 * i], h01, a3); c3 = __builtin_elementwise_fma(wa[3][2 * i + 1], h23, c3);
          }
          s0 = (a0[0] + a0[1]) + (c0[0] + c0[1]);
          s1 = (a1[0] + a1[1]) + (c1[0] + c1[1]);
          s2 = (a2[0] + a2[1]) + (c2[0] + c2[1]);
          s3 = (a3[0] + a3[1]) + (c3[0] + c3[1]);
          seq_row_sum4(s0, s1, s2, s3);
        }
#ifdef PK2_SEQ_PROFILE
        asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3));
#endif
        SQ_T(2);
        const float x = pre + (l16 == 0 ? s0 : l16 == 1 ? s1 : l16 == 2 ? s2 : s3);
        const float act = fmaf(act_a, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(act_s * x)), act_b);
        const float fg = seq_dpp<0x101>(act), gg = seq_dpp<0x102>(act), og = seq_dpp<0x103>(act);
        cstate = fg * cstate + act * gg;
        const float h = og * seq_tanh(cstate);
        if (unit_lane) seq_store(y_out, h);
        y_out += y_stride;
        SQ_T(3);
        if (gate_lane) outs[buf][out_idx] = act;
        if (unit_lane) outs[buf][64 + uw] = cstate;
        if (w == 3 && step > 0) {
          *gates_out = outs[buf ^ 1][lane];
          if (lane < 16) *cells_out = outs[buf ^ 1][64 + lane];
          gates_out += gates_stride; cells_out += cells_stride;
        }
        SQ_T(4);
      }
      __syncthreads();
      if (w == 3) {
        *gates_out = outs[(T - 1) & 1][lane];
        if (lane < 16) *cells_out = outs[(T - 1) & 1][64 + lane];
      }
      SQ_PRINT("lstm_fwd_seq2_xproj", "(poll | lds + barrier | product + row sums | gates + h store | lds hand-over, wave 3 traffic)", T);
      if (tid == 0 && rank == 0) __hip_atomic_fetch_add(&ctl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!seq_team_barrier(ctl, role, &nbar, s_i)) return;
  }
}

// WGRAD (lstm_bwd_seq2_wgrad): on top of the recurrence the workgroup keeps its 64 x 512 slice of
//   dW_hh[d] = sum_t dg_d[t]^T h_d[t -+ 1]        (the partner frame is the one the NEXT backward step visits)
// of its pair as MFMA accumulators: a step adds the rank-1 update dgl[64] x y[t_next][b][d*H ..][512] with 16
// v_mfma_f32_32x32x1_2b_f32 (the two 32-row blocks of the instruction = the two halves of dgl, A operand = dgl[lane] = the
// dg_own every wave reads anyway; an instruction per 32 columns, B operand = y[32 c + lane % 32] in both lane halves), four
// per wave: wave w owns columns 128 w .. 128 w + 127, 4 x 32 accumulator registers per lane.  Wave 1 brings the row of y
// in with its other prefetches (two 16-byte loads per lane, a step in flight, two steps ahead in an LDS ring of three).
// The MFMAs of a step are issued behind the step's mailbox stores (and wave 0's slot reset): nothing the chain waits on
// lies behind them.  At the end of the pair the slice goes to ws[task] with plain stores (one accumulator register = 32
// consecutive columns of two rows) and lstm_seq_wgrad_reduce adds the slices of the sequences in ascending order.
typedef float f32x32 __attribute__((ext_vector_type(32)));
struct SeqNoWgrad {};
__device__ __forceinline__ float (*seq_yring())[kSH] {     // (a function of its own: lstm_bwd_seq2 does not get the array)
  __shared__ __attribute__((aligned(16))) float ring[3][kSH];
  return ring;
}
template <bool WGRAD, typename WG>
__device__ __forceinline__ void lstm_bwd_seq2_body(const SeqBwdParams& p, SeqCtl* ctl, const WG& g) {
  constexpr int H = kSH, G4 = 4 * kSH;
  __shared__ __attribute__((aligned(16))) float dgl[64];               // this workgroup's dgates [gate * 16 + unit]
  __shared__ __attribute__((aligned(16))) float cst[3][16][8];         // [step % 3][unit]{dy, A, F, Ci, Cf, Cg, Co, -}: written two steps ahead
  float (*yring)[kSH] = nullptr;                                       // WGRAD: [step % 3] the partner frame's h, written two steps ahead
  if constexpr (WGRAD) yring = seq_yring();
  __shared__ int s_i[8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  SeqRole role;
  if (!seq_register(ctl, s_i, &role)) return;
  const int rank = role.rank, B = p.B, T = p.T, D = p.D;
  float* mail0 = p.mail + (size_t)role.team_index * kSeqMailFloats;
  const u32x4 sent = {kSeqSentinel, kSeqSentinel, kSeqSentinel, kSeqSentinel};
  const int row = lane >> 4, l16 = lane & 15;
  const bool pw_lane = w == 0 && l16 < 4;               // wave 0, lane j of row r: unit 4 r + j of the workgroup
  const int pw_unit = (4 * row + l16) & 15;
  const bool io = w == 1;                               // wave 1: prefetches and prepares the factors, writes d gx
  const bool io16 = io && lane < 16;
  unsigned nbar = 0;
  for (int iter = 0; iter <= kSeqMaxTasks; ++iter) {
    const int task = seq_next_task(ctl, role, iter, B * D, s_i);
    if (task < 0) return;
    const int b = task / D, d = task % D;
    // A lane pair owns one 16-byte granule of the partial d h -- columns k = 4 G .. 4 G + 3, G = 32 w + lane / 2, i.e. units
    // 4 (G % 4) .. of reader G / 4 -- and each lane of the pair half of the workgroup's 64 rows (lane % 2 = 0: gates i, f;
    // 1: gates g, o): W_hh[d][(gate)*H + 16*rank + unit][4 G + j] for its 32 rows.  The pair's sums meet by one DPP add per
    // value and the even lane stores the granule: one 16-byte store per lane pair and step.
    const int gidx = 32 * w + (lane >> 1), half = lane & 1;
    f32x2 wb[32][2];
    {
      const float* wbase = p.whh + (size_t)d * G4 * H + 4 * gidx;
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        const int rr = 32 * half + r;
        const f32x4 v = *reinterpret_cast<const f32x4*>(wbase + ((size_t)(rr >> 4) * H + 16 * rank + (rr & 15)) * H);
        wb[r][0] = f32x2{v[0], v[1]};
        wb[r][1] = f32x2{v[2], v[3]};
      }
    }
    float dcarry = 0.f;
    bool timed_out = false;
    // Everything addressed by time walks a pointer: the backward pass visits t = T - 1 - step (d = 0) or step (d = 1).
    const ptrdiff_t tdir = d == 0 ? -1 : 1;
    const size_t t0 = d == 0 ? (size_t)(T - 1) : 0;
    const ptrdiff_t dy_stride = tdir * (ptrdiff_t)((size_t)B * D * H), gates_stride = tdir * (ptrdiff_t)((size_t)B * G4);
    const ptrdiff_t cells_stride = tdir * (ptrdiff_t)((size_t)B * H), dgx_stride = tdir * (ptrdiff_t)((size_t)B * D * G4);
    const float* dy_in = p.dy + (t0 * B + b) * ((size_t)D * H) + (size_t)d * H + 16 * rank + (lane & 15);
    const float* gates_in = p.gates + (((size_t)d * T + t0) * B + b) * G4 + 16 * rank + (lane & 15);
    const float* cells_in = p.cells + (((size_t)d * T + t0) * B + b) * H + 16 * rank + (lane & 15);
    float* dgx_out = p.dgx + (t0 * B + b) * ((size_t)D * G4) + (size_t)d * G4 + (size_t)(lane >> 4) * H + 16 * rank + (lane & 15);
    // wave 1, lanes 0..15: the forward pass's values of step s + 4 (in flight) and of step s + 3
    // wave 1: the forward pass's values of the step after next but one, in flight for a whole step.  The loads are
    // unconditional, from pointers that stop at the last step (a load under a branch makes the compiler wait for it at the
    // join, i.e. at once; so does a register rotation: it copies the values just requested); lanes 16..63 of the wave
    // repeat the addresses of lanes 0..15.
    const float* cellsp_in = cells_in + (T > 1 ? cells_stride : 0);    // the cell of the time step before (forward order)
    float n_dy = 0.f, n_i = 0.f, n_f = 0.f, n_g = 0.f, n_o = 0.f, n_c = 0.f, n_cp = 0.f;
    // WGRAD: the partner frame of step s is t0 + (s + 1) tdir (none for the last step: the pointer stops at step T - 2's)
    const float* y_in = nullptr;
    f32x4 n_y0 = {0.f, 0.f, 0.f, 0.f}, n_y1 = n_y0;
    f32x32 acc0, acc1, acc2, acc3;
    if constexpr (WGRAD) {
      y_in = g.y + ((size_t)((ptrdiff_t)t0 + (T > 1 ? tdir : 0)) * B + b) * ((size_t)D * H) + (size_t)d * H + 4 * lane;
#pragma unroll
      for (int i = 0; i < 32; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; acc2[i] = 0.f; acc3[i] = 0.f; }
    }
    auto load_pw = [&](int step_) {                      // (called for step_ = 0, 1, 2, ...: the pointers walk along)
      const bool more = step_ + 1 < T, more2 = step_ + 2 < T;
      if constexpr (WGRAD) {
        n_y0 = *reinterpret_cast<const f32x4*>(y_in);
        n_y1 = *reinterpret_cast<const f32x4*>(y_in + 256);
        y_in += more2 ? dy_stride : 0;                   // (y and dy have the same frame stride)
      }
      n_dy = *dy_in;
      n_i = gates_in[0]; n_f = gates_in[H]; n_g = gates_in[2 * H]; n_o = gates_in[3 * H];
      n_c = *cells_in;
      n_cp = *cellsp_in;
      dy_in += more ? dy_stride : 0; gates_in += more ? gates_stride : 0; cells_in += more ? cells_stride : 0;
      cellsp_in += more2 ? cells_stride : 0;
    };
    auto put_factors = [&](int step_, int slot) {        // from the values in flight (step step_) into cst[slot]
      const float cp = step_ == T - 1 ? 0.f : n_cp;      // the last step of the backward pass has no previous cell
      if constexpr (WGRAD) {
        *reinterpret_cast<f32x4*>(&yring[slot][4 * lane]) = n_y0;
        *reinterpret_cast<f32x4*>(&yring[slot][256 + 4 * lane]) = n_y1;
      }
      if (io16) {
        const float tc = seq_tanh(n_c);
        float* o = &cst[slot][lane][0];
        *reinterpret_cast<f32x4*>(o) = f32x4{n_dy, n_o * (1.f - tc * tc), n_f, n_g * n_i * (1.f - n_i)};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{cp * n_f * (1.f - n_f), n_i * (1.f - n_g * n_g), tc * n_o * (1.f - n_o), 0.f};
      }
    };
    if (io) {
      load_pw(0); put_factors(0, 0);
      load_pw(1); put_factors(1, 1);
      load_pw(2);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): W_hh is there before the loop (no waits for it inside)
    __syncthreads();
    // the mailbox of the step: [step % 8][reader][writer][16 units]; wave 0 reads [.][rank][writer l16 (+ 16)][units 4 row ..]
    float* mail_rd = mail0 + (size_t)rank * (kSWgs * 16) + (size_t)l16 * 16 + 4 * row;
    float* mail_wr = mail0 + ((size_t)(gidx >> 2) * kSWgs + rank) * 16 + 4 * (gidx & 3);  // peer G/4 reads [writer = rank][units 4 (G%4) ..]
    constexpr int kBox = kSWgs * kSWgs * 16;
    int s3 = 0;                                          // step % 3
    float bias_sum = 0.f;                                // wave 1: sum over the frames of its lane's d gate (the bias gradient)
    SeqSpin spin(ctl);
    spin.limit = 10 * kSeqSpinTicks;      // (as in the forward kernel)
    SQ_T0();
    for (int step = 0; step < T; ++step) {
      if (step == 2) { spin.limit = kSeqSpinTicks; spin.t0 = 0; }
      const int s3n = s3 == 2 ? 0 : s3 + 1;
      const int m8 = step & (kSeqMailDepth - 1), m8n = (step + 1) & (kSeqMailDepth - 1);
      if (w == 0) {
        // the step's factors (written by wave 1 two steps ago: a barrier lies between)
        const f32x4 fa = *reinterpret_cast<const f32x4*>(&cst[s3][pw_unit][0]);
        const f32x4 fb = *reinterpret_cast<const f32x4*>(&cst[s3][pw_unit][4]);
        // ---- gather the 32 partials of d h for the own 16 units (written by the peers during the previous step) --------
        f32x4 r4 = {0.f, 0.f, 0.f, 0.f};
        if (step > 0) {
          float* src = mail_rd + m8 * kBox;
          u32x4 v0, v1;
#ifdef PK2_SEQ_PROFILE
          { const long long c0_ = clock64(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); sq_acc_[4] += clock64() - c0_; }   // own stores acknowledged
          bool first_ = true; const long long c1_ = clock64();
#endif
          for (;;) {
            asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:1024 sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(v0), "=&v"(v1) : "v"(src) : "memory");
#ifdef PK2_SEQ_PROFILE
            if (first_) { sq_acc_[5] += clock64() - c1_; first_ = false; }
#endif
            if (!seq_has_sentinel(v0) && !seq_has_sentinel(v1)) break;
            if (spin.expired()) { timed_out = true; break; }
          }
#ifdef PK2_SEQ_PROFILE
          sq_acc_[6] += clock64() - c1_;           // the whole poll loop
#endif
          float q0 = __uint_as_float(v0.x) + __uint_as_float(v1.x), q1 = __uint_as_float(v0.y) + __uint_as_float(v1.y);
          float q2 = __uint_as_float(v0.z) + __uint_as_float(v1.z), q3 = __uint_as_float(v0.w) + __uint_as_float(v1.w);
          seq_row_sum4(q0, q1, q2, q3);
          r4 = f32x4{q0, q1, q2, q3};
        }
        SQ_T(0);
        if (timed_out) s_i[3] = 1;
        // ---- gate derivatives of the own units: lane j of row r, unit 4 r + j -------------------------------------------
        const float rec = l16 == 0 ? r4[0] : l16 == 1 ? r4[1] : l16 == 2 ? r4[2] : r4[3];
        const float dh = fa[0] + rec;
        const float dcv = fmaf(dh, fa[1], dcarry);
        dcarry = dcv * fa[2];
        if (pw_lane) {
          dgl[pw_unit] = dcv * fa[3]; dgl[16 + pw_unit] = dcv * fb[0]; dgl[32 + pw_unit] = dcv * fb[1]; dgl[48 + pw_unit] = dh * fb[2];
        }
        SQ_T(1);
      }
      seq_lds_barrier();
      SQ_T(2);
      if (s_i[3]) {              // loud failure: the gradient of this layer turns NaN
        if (tid == 0) p.dgx[(size_t)d * G4 + 16 * rank] = __int_as_float(0x7fc00000);
        return;
      }
      // WGRAD: the wave's 4 x 32 columns of the partner frame.  Requested in front of dg_own, whose wait they share (a wait
      // of their own in front of the product would put an LDS round trip on the chain); the mailbox stores' memory
      // clobber keeps the reads above them.
      float yb0 = 0.f, yb1 = 0.f, yb2 = 0.f, yb3 = 0.f;
      if constexpr (WGRAD) {
        const float* yq = &yring[s3][128 * w + (lane & 31)];
        yb0 = yq[0]; yb1 = yq[32]; yb2 = yq[64]; yb3 = yq[96];
      }
      float dg_own = dgl[lane];                // (wave 1 writes it out behind the product; wave 0 may be a step ahead by then:
      asm volatile("" : "+v"(dg_own));         // the read must not sink below the mailbox stores)
      if (step < T - 1) {
        // ---- own 64 rows of dgates x own W_hh rows: the lane's two columns -------------------------------------------------
        f32x2 a0 = {0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0, c0 = a0, c1 = a0, c2 = a0, c3 = a0;     // eight independent chains
        f32x4 dva[8];                                       // all eight reads in flight before the first FMA
#pragma unroll
        for (int r4i = 0; r4i < 8; ++r4i) dva[r4i] = *reinterpret_cast<const f32x4*>(&dgl[32 * half + 4 * r4i]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r4i = 0; r4i < 8; ++r4i) {
          const f32x4 dv = dva[r4i];
          a0 = __builtin_elementwise_fma(f32x2{dv[0], dv[0]}, wb[4 * r4i][0], a0);     c0 = __builtin_elementwise_fma(f32x2{dv[0], dv[0]}, wb[4 * r4i][1], c0);
          a1 = __builtin_elementwise_fma(f32x2{dv[1], dv[1]}, wb[4 * r4i + 1][0], a1); c1 = __builtin_elementwise_fma(f32x2{dv[1], dv[1]}, wb[4 * r4i + 1][1], c1);
          a2 = __builtin_elementwise_fma(f32x2{dv[2], dv[2]}, wb[4 * r4i + 2][0], a2); c2 = __builtin_elementwise_fma(f32x2{dv[2], dv[2]}, wb[4 * r4i + 2][1], c2);
          a3 = __builtin_elementwise_fma(f32x2{dv[3], dv[3]}, wb[4 * r4i + 3][0], a3); c3 = __builtin_elementwise_fma(f32x2{dv[3], dv[3]}, wb[4 * r4i + 3][1], c3);
        }
        a0 = (a0 + a1) + (a2 + a3); c0 = (c0 + c1) + (c2 + c3);
        float g0 = a0[0], g1 = a0[1], g2 = c0[0], g3 = c0[1];
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
                     : "+v"(g0), "+v"(g1), "+v"(g2), "+v"(g3));
        if (half == 0) {
          const f32x4 gv = {g0, g1, g2, g3};
          u32x4 gu4;
          __builtin_memcpy(&gu4, &gv, 16);
          seq_store16(mail_wr + m8n * kBox, gu4);
        }
      }
      // The mailbox slot read in this step is free again: its reset goes out behind the step's own partials (issuing the
      // two stores takes ~300 clocks, which the poll of the next step has to spare) and has until the slot's next use, seven
      // steps on, to land.
      if (w == 0 && step > 0) {
        seq_store16(mail_rd + m8 * kBox, sent);
        seq_store16(mail_rd + m8 * kBox + 256, sent);
      }
      SQ_T(3);
      if constexpr (WGRAD) {
        if (step < T - 1) {      // behind the hand-over: the step's rank-1 update of the pair's dW_hh slice
          acc0 = __builtin_amdgcn_mfma_f32_32x32x1f32(dg_own, yb0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x1f32(dg_own, yb1, acc1, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x1f32(dg_own, yb2, acc2, 0, 0, 0);
          acc3 = __builtin_amdgcn_mfma_f32_32x32x1f32(dg_own, yb3, acc3, 0, 0, 0);
        }
        SQ_T(7);
      }
      if (io) {                  // behind the hand-over: d gx of the step to HBM, the factors two steps ahead, the prefetch
        *dgx_out = dg_own;
        dgx_out += dgx_stride;
        bias_sum += dg_own;
        put_factors(step + 2, s3 == 0 ? 2 : s3 - 1);                   // slot (step + 2) % 3, from the loads of a step ago
        load_pw(step + 3);
      }
      s3 = s3n;
    }
    // the bias gradients (b_ih and b_hh receive the same sum) of this (sequence, direction): one atomic per gate row
    if (io && p.dbias_ih) {
      const size_t at = (size_t)d * G4 + (size_t)(lane >> 4) * H + 16 * rank + (lane & 15);
      atomicAdd(p.dbias_ih + at, bias_sum);
      if (p.dbias_hh) atomicAdd(p.dbias_hh + at, bias_sum);
    }
    if constexpr (WGRAD) {
      // The pair's slice: accumulator register v of column group c holds, in lane l, row 32 (v / 16) + 8 ((v % 16) / 4) +
      // 4 (l / 32) + v % 4 of dgl's 64 and column 128 w + 32 c + l % 32; dgl's row i is row (i / 16) H + 16 rank + i % 16
      // of dW_hh[d].
      float* wsp = g.ws + (size_t)task * G4 * H + 128 * w + (lane & 31);
#pragma unroll
      for (int v = 0; v < 32; ++v) {
        const int i = 32 * (v >> 4) + 8 * ((v & 15) >> 2) + 4 * (lane >> 5) + (v & 3);
        float* o = wsp + ((size_t)(i >> 4) * H + 16 * rank + (i & 15)) * H;
        o[0] = acc0[v]; o[32] = acc1[v]; o[64] = acc2[v]; o[96] = acc3[v];
      }
    }
    SQ_PRINT(WGRAD ? "lstm_bwd_seq2_wgrad" : "lstm_bwd_seq2", "(wave 0: mailbox poll + row sums | gate derivatives | lds barrier | product + mailbox stores || inside the poll: own stores acknowledged | first poll round trip | poll loop | wgrad: the MFMAs' issue)", T);
    if (tid == 0 && rank == 0) __hip_atomic_fetch_add(&ctl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!seq_team_barrier(ctl, role, &nbar, s_i)) return;     // nobody writes a mailbox of the next pair before everybody has read the last of this one
  }
}

// A launch in which a poll timed out (or a pair was never finished) must not pass for a result: the forward
// pass keeps its NaN sentinels in y, but the backward pass would leave dgx -- freshly allocated memory -- partly
// unwritten.  One workgroup after every persistent launch turns the launch's output into NaN in that case and raises a
// sticky flag (the control block itself is cleared by the next launch) that pk2_lstm_persist_status reports.
// (round 5: the check also leaves the control block zeroed for the next launch on this stream -- one hipMemsetAsync, i.e.
// one fill kernel, less per recurrence launch: six per LF-MMI step)
// This separate kernel checks the first forward launch on a device; every other launch folds the check in (seq_exit_check).
__global__ void lstm_seq_check(SeqCtl* ctl, unsigned pairs, float* out, size_t n, unsigned* sticky, unsigned* guard_dev, unsigned* guard_host) {
  const bool good = ctl->abort == 0u && ctl->done == pairs;
  __syncthreads();
  for (unsigned i = threadIdx.x; i < sizeof(SeqCtl) / sizeof(unsigned); i += blockDim.x) reinterpret_cast<unsigned*>(ctl)[i] = 0u;
  if (good) return;
  if (threadIdx.x == 0) { *sticky = 1u; persist_guard_raise(guard_dev, guard_host); }
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) out[i] = __uint_as_float(0x7fc00000u);
}

// Round 6: the check rides in the recurrence launch.  Every workgroup counts itself out; the last one to leave sees the
// control block in its final state (every other workgroup's atomics are in L2 before its exit count), does what
// lstm_seq_check does -- verdict, control block zeroed for the next launch, on failure the sticky flag, the guard and the NaN
// poison -- and the step has six launches less.  (first use on a device: `fold` = 0, the host reads the control block itself)
// `mail` (backward pass): an aborted launch leaves consumed and unconsumed hand-overs in the mailboxes, which the next
// launch would read as valid ones -- the same workgroup fills them with sentinels again, so that a caller who
// lowers the guard (pk2_persist_guard_clear) and carries on does not compute on stale words.
struct SeqExit { unsigned pairs; int fold; float* out; size_t n; unsigned* sticky; unsigned* guard_dev; unsigned* guard_host; float* mail; size_t mail_n; };
__device__ __forceinline__ void seq_exit_check(SeqCtl* ctl, const SeqExit& x) {
  if (!x.fold) return;
  __shared__ unsigned s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&ctl->exited, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  const bool good = seq_load_u(&ctl->abort) == 0u && seq_load_u(&ctl->done) == x.pairs && x.fold != 2;     // (fold = 2: test hook)
  __syncthreads();
  for (unsigned i = threadIdx.x; i < sizeof(SeqCtl) / sizeof(unsigned); i += blockDim.x) reinterpret_cast<unsigned*>(ctl)[i] = 0u;
  if (good) return;
  if (threadIdx.x == 0) { if (x.fold != 2) *x.sticky = 1u; persist_guard_raise(x.guard_dev, x.guard_host); }
  for (size_t i = threadIdx.x; i < x.n; i += blockDim.x) x.out[i] = __uint_as_float(0x7fc00000u);
  for (size_t i = threadIdx.x; i < x.mail_n; i += blockDim.x) x.mail[i] = __uint_as_float(kSeqSentinel);
}
__global__ void __launch_bounds__(256) lstm_fwd_seq2(SeqFwdParams p, SeqCtl* ctl, SeqExit x) {
  lstm_fwd_seq2_body(p, ctl);
  seq_exit_check(ctl, x);
}
__global__ void __launch_bounds__(256) lstm_bwd_seq2(SeqBwdParams p, SeqCtl* ctl, SeqExit x) {
  lstm_bwd_seq2_body<false>(p, ctl, SeqNoWgrad());
  seq_exit_check(ctl, x);
}
__global__ void __launch_bounds__(256) lstm_bwd_seq2_wgrad(SeqBwdParams p, SeqCtl* ctl, SeqExit x, SeqWgradParams g) {
  lstm_bwd_seq2_body<true>(p, ctl, g);
  seq_exit_check(ctl, x);
}

// (512 threads: two waves per SIMD, at most 256 registers per lane; one workgroup per CU by its LDS)
template <int K>
__global__ void __launch_bounds__(512) lstm_fwd_seq2_xproj(SeqFwdParams p, SeqXprojParams xp, SeqCtl* ctl, SeqExit x) {
  lstm_fwd_seq2_xproj_body<K>(p, xp, ctl);
  seq_exit_check(ctl, x);
}

// dwhh[d][r][k] += sum over the sequences b = 0 .. B - 1, in this order, of ws[b D + d][r][k]: the result is fixed by
// construction (no float atomics).  A launch that gave up has left slices unwritten and the sticky word of its stream set
// (seq_exit_check, which runs before this kernel starts): then dwhh turns NaN like dgx.  The word is the one
// pk2_lstm_persist_status reports and is never cleared, not by pk2_persist_guard_clear either: once a recurrence launch on
// this stream, forward or backward, has given up, EVERY later fused call writes NaN into dwhh although its dgx is valid -- a
// process that lowers the guard and carries on sets PK2_LSTM_SEQ_WGRAD=0 (the caller's product, from the valid dgx).
__global__ void __launch_bounds__(256) lstm_seq_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dwhh, int B, int D,
                                                             const unsigned* __restrict__ sticky) {
  constexpr size_t kSlice = (size_t)4 * kSH * kSH;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;    // element of dwhh: the grid covers the D slices exactly
  if (*sticky != 0u) {
    dwhh[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  const float* in = ws + i;                                   // (task = b D + d: sequence b's slices lie D slices further on)
  float sum = in[0];
  for (int b = 1; b < B; ++b) sum += in[(size_t)b * D * kSlice];
  dwhh[i] += sum;
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct SeqScratch { SeqCtl* ctl = nullptr; float* mail = nullptr; unsigned* sticky = nullptr; PersistGuard guard;
                    int mail_clean_teams = 0;         // mailboxes of that many teams per XCD are known to hold only sentinels
                    bool ctl_clean = false; };        // the last launch's check kernel has zeroed the control block
static std::map<DevStream, SeqScratch> g_seq_scratch;
static PersistFamily g_seq("lstm_seq");

// pk2_persist_guard_clear: whatever an aborted launch left behind, the next backward launch fills every mailbox again
// (belt and braces next to the refill by the folded check: a launch that was killed never reached it).
static void seq_mail_dirty() { for (auto& kv : g_seq_scratch) { kv.second.mail_clean_teams = 0; kv.second.ctl_clean = false; } }

static int seq_scratch(hipStream_t stream, SeqScratch** out) {
  static const bool hooked = (persist_guard_on_clear(seq_mail_dirty), true);
  (void)hooked;
  SeqScratch& sc = g_seq_scratch[dev_stream(stream)];
  if (!sc.ctl) PK2_HIP(hipMalloc(reinterpret_cast<void**>(&sc.ctl), sizeof(SeqCtl)));
  if (!sc.mail) PK2_HIP(hipMalloc(reinterpret_cast<void**>(&sc.mail), (size_t)8 * kSeqTeams * kSeqMailFloats * sizeof(float)));
  if (!sc.sticky) { int rc = g_seq.new_sticky(stream, &sc.sticky); if (rc) return rc; }
  if (!sc.guard.dev) { int rc = persist_guard(&sc.guard); if (rc) return rc; }
  *out = &sc;
  return PK2_OK;
}

// Teams per XCD of a launch: with more than 8 pairs a second team per XCD takes its own pairs from the queue at the same
// time (two workgroups per CU; a recurrence is latency-bound, two of them interleave almost for free).
static int seq_teams(int pairs) { return std::max(1, std::min(2, (pairs + 7) / 8)); }

bool lstm_seq_wanted(int B, int H, int D) {
  const char* env = getenv("PK2_LSTM_SEQ");
  if (env && atoi(env) == 0) return false;
  // (up to 4 pairs per XCD one after the other; larger batches are better served by the batched step kernels)
  if (!g_seq.usable() || H != kSH || B < 1 || B * D > 32 || (D != 1 && D != 2)) return false;
  return device_cu_count() == 8 * kSWgs;
}

// The forward launch protocol, shared by lstm_fwd_seq2 and lstm_fwd_seq2_xproj (xp != null: `teams` teams per XCD of its
// 512-thread workgroups): control block, y pre-filled with the sentinel, the folded exit check (or, on first use of a device,
// the host's verdict and the separate check kernel).
static int seq_fwd_launch(const SeqFwdParams& p, const SeqXprojParams* xp, int teams, int H, hipStream_t stream, bool* ran) {
  *ran = false;
  const int B = p.B, T = p.T, D = p.D;
  float* y = p.y;
  SeqScratch* sc = nullptr;
  int rc = seq_scratch(stream, &sc);
  if (rc) return rc;
  if (!sc->ctl_clean) PK2_HIP(hipMemsetAsync(sc->ctl, 0, sizeof(SeqCtl), stream));
  sc->ctl_clean = false;
  PK2_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(y), (int)kSeqSentinel, (size_t)T * B * D * H, stream));
  // (the first launch on a device is checked by the host below and by the separate check kernel: no folded check)
  const bool fold = g_seq.verified();
  // (test hook, read per call: PK2_LSTM_SEQ_TEST_FAIL=1 makes the folded check of a forward launch behave as if a poll had timed out)
  const char* tf_e = getenv("PK2_LSTM_SEQ_TEST_FAIL");
  const int fold_mode = fold ? ((tf_e && atoi(tf_e) == 1) ? 2 : 1) : 0;
  const SeqExit ex{(unsigned)(B * D), fold_mode, y, (size_t)T * B * D * H, sc->sticky, sc->guard.dev, sc->guard.host_dev, nullptr, (size_t)0};
  if (!xp)
    hipLaunchKernelGGL(lstm_fwd_seq2, dim3(8 * kSWgs * teams), dim3(256), 0, stream, p, sc->ctl, ex);
  else if (xp->K == 80)
    hipLaunchKernelGGL(lstm_fwd_seq2_xproj<80>, dim3(8 * kSWgs * teams), dim3(512), 0, stream, p, *xp, sc->ctl, ex);
  else
    hipLaunchKernelGGL(lstm_fwd_seq2_xproj<1024>, dim3(8 * kSWgs * teams), dim3(512), 0, stream, p, *xp, sc->ctl, ex);
  PK2_LAUNCH_CHECK();
  bool ok = false;                                // first use on this device: every pair done, nobody timed out?
  rc = g_seq.verify_first_use(&sc->ctl->abort, &sc->ctl->done, (unsigned)(B * D), stream, &ok);
  if (rc || !ok) return rc;
  if (!fold)
    hipLaunchKernelGGL(lstm_seq_check, dim3(1), dim3(1024), 0, stream, sc->ctl, (unsigned)(B * D), y, (size_t)T * B * D * H, sc->sticky, sc->guard.dev, sc->guard.host_dev);
  sc->ctl_clean = true;
  *ran = true;
  return PK2_OK;
}

int lstm_fwd_seq_launch(const float* gx, const float* whh, const float* bhh, int B, int T, int H, int D, float* y,
                        float* gates, float* cells, hipStream_t stream, bool* ran) {
  const SeqFwdParams p{gx, whh, bhh, y, gates, cells, B, T, D};
  return seq_fwd_launch(p, nullptr, seq_teams(B * D), H, stream, ran);
}

// lstm_fwd_seq2_xproj keeps 156 KB of LDS and eight waves: it is used only where the runtime says that a workgroup of
// either instantiation fits a CU (asked once per device, as for lstm_bwd_seq2_wgrad).
static bool seq_xproj_resident() {
  static std::map<int, bool> fit;
  const int dev = current_device();
  auto it = fit.find(dev);
  if (it == fit.end()) {
    int n80 = 0, n1024 = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n80, lstm_fwd_seq2_xproj<80>, 512, 0) != hipSuccess) { (void)hipGetLastError(); n80 = 0; }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1024, lstm_fwd_seq2_xproj<1024>, 512, 0) != hipSuccess) { (void)hipGetLastError(); n1024 = 0; }
    it = fit.emplace(dev, n80 >= 1 && n1024 >= 1).first;
  }
  return it->second;
}

// PK2_LSTM_SEQ_XPROJ, read per call: 0 = the caller multiplies as before; 1 = fused for up to 8 pairs (one team per XCD, a
// workgroup per CU); 2 = also for 9 .. 32 pairs, which then queue up behind 8 teams instead of 16 (for the tests: it is
// what makes a team compute a second pair's projections over the ring of the first).
// Not fused (*ran = false, nothing launched or written): a device whose first forward launch has not been verified yet,
// in_size other than 80 and 1024, operands that are not 16-byte aligned.
int lstm_fwd_seq_xproj_launch(const float* inp, int in_size, const float* wih, const float* bih, const float* whh, const float* bhh,
                              int B, int T, int H, int D, float* y, float* gates, float* cells, hipStream_t stream, bool* ran) {
  *ran = false;
  const char* xe = getenv("PK2_LSTM_SEQ_XPROJ");
  const int mode = xe ? atoi(xe) : 1;
  if (mode == 0 || !g_seq.verified() || (in_size != 80 && in_size != 1024)) return PK2_OK;
  if (B * D > 8 && mode != 2) return PK2_OK;
  if ((reinterpret_cast<uintptr_t>(inp) | reinterpret_cast<uintptr_t>(wih) | reinterpret_cast<uintptr_t>(bih)) % 16 != 0) return PK2_OK;
  if (!seq_xproj_resident()) return PK2_OK;
  const SeqFwdParams p{nullptr, whh, bhh, y, gates, cells, B, T, D};
  const SeqXprojParams xp{inp, wih, bih, in_size};
  return seq_fwd_launch(p, &xp, 1, H, stream, ran);
}

// The team protocol needs every launched workgroup resident: lstm_bwd_seq2_wgrad is used only when the runtime says that
// `teams` of its workgroups fit a CU (asked once per device; nothing rests on a register count read off a listing).
static bool seq_wgrad_resident(int teams) {
  static std::map<int, int> fit;
  const int dev = current_device();
  auto it = fit.find(dev);
  if (it == fit.end()) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lstm_bwd_seq2_wgrad, 256, 0) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    it = fit.emplace(dev, n).first;
  }
  return it->second >= teams;
}

// PK2_LSTM_SEQ_WGRAD, read per call: 0 = the caller multiplies as before; 2 = where the two teams per XCD that more than 8
// pairs ask for are not resident, the fused kernel with ONE team per XCD (the pairs queue up behind 8 teams instead of 16:
// for measuring that trade, and for the tests -- it is what makes a team flush and clear its accumulators between pairs).
static int seq_wgrad_mode() {
  const char* we = getenv("PK2_LSTM_SEQ_WGRAD");
  return we ? atoi(we) : 1;
}
// Teams per XCD of a fused launch; 0: the launch is not fused.
static int seq_wgrad_teams(int pairs) {
  const int mode = seq_wgrad_mode();
  if (mode == 0) return 0;
  if (seq_wgrad_resident(seq_teams(pairs))) return seq_teams(pairs);
  return (mode == 2 && seq_wgrad_resident(1)) ? 1 : 0;
}

// (0 where no launch of this shape would be fused: the caller then allocates nothing)
size_t lstm_seq_wgrad_workspace_floats(int B, int H, int D) {
  return (lstm_seq_wanted(B, H, D) && seq_wgrad_teams(B * D) > 0) ? (size_t)B * D * 4 * H * H : 0;
}

int lstm_bwd_seq_launch(const float* dy, const float* whh, const float* gates, const float* cells, int B, int T, int H,
                        int D, float* dgx, hipStream_t stream, bool* ran, float* dbias_ih, float* dbias_hh, bool* bias_done,
                        SeqWgradCall* wgrad) {
  *ran = false;
  if (bias_done) *bias_done = false;
  if (wgrad) wgrad->done = false;
  if (!g_seq.verified()) return PK2_OK;           // the forward pass verifies the device first
  SeqScratch* sc = nullptr;
  int rc = seq_scratch(stream, &sc);
  if (rc) return rc;
  if (!sc->ctl_clean) PK2_HIP(hipMemsetAsync(sc->ctl, 0, sizeof(SeqCtl), stream));
  sc->ctl_clean = false;
  // Every reader resets the slots it has read, so a launch that completes leaves the mailboxes as it found them: all
  // sentinels.  They are filled once (and again when a launch needs more teams than have been filled); a launch that
  // gave up raises the guard, which stops training anyway (persist_guard.h).
  // The recurrent weight gradient from inside the recurrence.  T = 1 has no partner frame: nothing to add, and nothing is
  // launched for it (done all the same, unless switched off).
  int teams = seq_teams(B * D);
  bool fused = false, wgrad_trivial = false;
  if (wgrad && wgrad->y && wgrad->dwhh && reinterpret_cast<uintptr_t>(wgrad->y) % 16 == 0) {
    if (T == 1) {
      wgrad_trivial = seq_wgrad_mode() != 0;
    } else if (wgrad->ws) {
      const int wt = seq_wgrad_teams(B * D);
      if (wt > 0) { fused = true; teams = wt; }
    }
  }
  if (sc->mail_clean_teams < teams) {
    PK2_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sc->mail), (int)kSeqSentinel, (size_t)8 * teams * kSeqMailFloats, stream));
    sc->mail_clean_teams = teams;
  }
  SeqBwdParams p{dy, whh, gates, cells, dgx, sc->mail, B, T, D, dbias_ih, dbias_hh};
  if (bias_done) *bias_done = dbias_ih != nullptr;
  const SeqExit ex{(unsigned)(B * D), 1, dgx, (size_t)T * B * D * 4 * H, sc->sticky, sc->guard.dev, sc->guard.host_dev, sc->mail,
                   (size_t)8 * kSeqTeams * kSeqMailFloats};
  if (fused) {
    const SeqWgradParams g{wgrad->y, wgrad->ws};
    hipLaunchKernelGGL(lstm_bwd_seq2_wgrad, dim3(8 * kSWgs * teams), dim3(256), 0, stream, p, sc->ctl, ex, g);
    PK2_LAUNCH_CHECK();
    hipLaunchKernelGGL(lstm_seq_wgrad_reduce, dim3((unsigned)((size_t)D * 4 * H * H / 256)), dim3(256), 0, stream, wgrad->ws,
                       wgrad->dwhh, B, D, sc->sticky);
  } else {
    hipLaunchKernelGGL(lstm_bwd_seq2, dim3(8 * kSWgs * teams), dim3(256), 0, stream, p, sc->ctl, ex);
  }
  PK2_LAUNCH_CHECK();
  if (wgrad) wgrad->done = fused || wgrad_trivial;
  sc->ctl_clean = true;
  *ran = true;
  return PK2_OK;
}

int lstm_seq_status(unsigned* abort_flag) {
  unsigned any = g_seq.any_gave_up();
  for (auto& kv : g_seq_scratch) {           // and a launch that gave up whose check has not zeroed the control block yet
    unsigned live = 0;
    if (kv.second.ctl && hipMemcpy(&live, &kv.second.ctl->abort, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess) any |= live;
  }
  *abort_flag = any;
  return PK2_OK;
}

}  // namespace pk2
