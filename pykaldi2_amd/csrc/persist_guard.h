// What happens after a persistent kernel gave up: every persistent launch is followed by a one-workgroup check
// kernel that, when a poll of the launch timed out (or a task never finished), poisons the launch's output with NaN and
// raises a flag of its own subsystem.  That alone leaves the damage to the caller: a CE step has no Kaldi-style NaN guard,
// and Adam would write the NaN into every weight.  So the check kernels also raise this process-wide guard:
//  * a word in device memory that the optimiser kernels (optim.hip) read -- while it is set they leave the parameters and
//    their moments untouched, whatever the gradients hold;
//  * a word in host-mapped memory that the host reads WITHOUT synchronising (pk2_persist_guard_status): the Python
//    optimisers raise at the first step() that sees it.
// One guard per device (a process that drives two GPUs gets two).
#pragma once
#include <vector>

#include "common.h"

namespace pk2 {

struct PersistGuard {
  unsigned* dev = nullptr;        // device memory: read by kernels
  unsigned* host_dev = nullptr;   // device address of the host-mapped word: written by the check kernels
  volatile unsigned* host = nullptr;
  // Verdicts of the COLLECTIVE guard (several ranks, round 5): ring of kGuardRing host-mapped words, word[stamp % ring] =
  // (stamp << 1) | raised, written by pk2_persist_guard_import after the ranks exchanged their guard words, so that every
  // rank reads the same verdict for the same step and stops at the same step (pykaldi2_amd/hvd.py).
  unsigned* ring_dev = nullptr;
  volatile unsigned* ring = nullptr;
};
constexpr unsigned kGuardRing = 8;

// The guard of the current device (created on first use); PK2_OK or an error code.
int persist_guard(PersistGuard* out);
// `fn` runs whenever pk2_persist_guard_clear lowers a guard: scratch state an aborted launch may have left behind is
// marked for re-initialisation (lstm_persist_seq.hip: the backward mailboxes).
void persist_guard_on_clear(void (*fn)());

// The same for a check kernel whose launch goes ahead whatever happens: null pointers when the guard cannot be had
// (persist_guard_raise accepts them).
PersistGuard persist_guard_or_null();

__device__ __forceinline__ void persist_guard_raise(unsigned* dev, unsigned* host_dev) {
  if (dev) *dev = 1u;
  if (host_dev) __hip_atomic_store(host_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- host protocol of a persistent launch ("host protocol of a persistent launch") ----------------------------
// Compute units of the current device (cached per device), 0 when it cannot be asked.  The persistent kernels form their
// teams for 8 XCDs x 32 CUs; every family compares with its own constant.
int device_cu_count();

// Raises `kernel`'s dynamic-LDS limit to `bytes` the first time it is asked for on the current device (a second
// GPU in the same process is configured again); every template instance is a kernel of its own.  Returns from the caller
// with PK2_ERR_HIP on an error, which is then tried again by the next call.
int raise_dyn_lds_once(const void* kernel, int bytes, const char* file, int line);
#define PK2_DYN_LDS_ONCE(kernel, bytes)                                                                             \
  do {                                                                                                              \
    int rc_ = pk2::raise_dyn_lds_once(reinterpret_cast<const void*>(&kernel), (bytes), __FILE__, __LINE__);         \
    if (rc_) return rc_;                                                                                            \
  } while (0)

// One per kernel family.  The verdict is kept per device: -1 not tried yet, 0 unusable (the family's *_wanted function says
// no from then on), 1 verified.
class PersistFamily {
 public:
  explicit PersistFamily(const char* name) : name_(name), verdict_(-1) {}
  int verdict() { return verdict_.ref(); }
  bool usable() { return verdict_.ref() != 0; }
  bool verified() { return verdict_.ref() == 1; }
  // Behind the first launch on a device, before its check kernel: waits for the stream and reads the two words every
  // control block has.  *ok = nobody timed out and all `expected_done` tasks were finished; that is the verdict from then
  // on, and with a verdict known the call does nothing but report it.  When it is not ok the caller falls back (and keeps
  // doing so).  A HIP error is reported as "<name>: ..." and leaves the device untried.
  int verify_first_use(const unsigned* abort_dev, const unsigned* done_dev, unsigned expected_done, hipStream_t stream, bool* ok);
  // The sticky "some launch gave up" word the family's check kernels set: a new, cleared word for a scratch block (one per
  // device and stream), and the OR of all words handed out so far (copies them back: synchronise first).
  int new_sticky(hipStream_t stream, unsigned** out);
  unsigned any_gave_up();

 private:
  const char* name_;
  PerDevice<int> verdict_;
  std::vector<unsigned*> sticky_;
};

}  // namespace pk2
