"""Transducer loss + gradients timing on the frame counts of the LF-MMI bench minibatch (146 / 539 / 569 / 159), V = 43 and
V = 5768, seeded transcripts of one label per 8 frames, logits N(0, 2) for am and lm:

  transducer.transducer_loss_and_grad (csrc/transducer.hip: seven launches), timed with events, a warm-up call first;
  median / min / max of --reps.  There is no earlier path to compare against: these are records, not pass marks.

Next to the time: the workspace bytes of the call and the bytes of the float32 [N, T, U + 1, V] joint that was not built.
The per-launch kernel times (td_lattice over the T + U diagonals of the longest utterance gives the time per diagonal) come
from the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o td -- python tools/transducer_time.py
Prints one JSON line per V; with --out FILE appends them there."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import _lib, transducer  # noqa: E402

FRAMES = [146, 539, 569, 159]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    for V in (43, 5768):
        rng = np.random.default_rng(V)
        blank = V - 1
        labels = [rng.integers(0, V - 1, size=T // 8).tolist() for T in FRAMES]
        U1 = max(map(len, labels)) + 1
        am = torch.from_numpy(rng.normal(0, 2, size=(4, max(FRAMES), V)).astype(np.float32)).to(dev)
        lm = torch.from_numpy(rng.normal(0, 2, size=(4, U1, V)).astype(np.float32)).to(dev)
        transducer.transducer_loss_and_grad(am, lm, FRAMES, labels, blank)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss, _, _, status = transducer.transducer_loss_and_grad(am, lm, FRAMES, labels, blank)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        host = torch.from_numpy(transducer.pack(FRAMES, labels, max(FRAMES), U1, V, blank))
        out = dict(frames=FRAMES, V=V, labels=[len(s) for s in labels], reps=reps, median_ms=round(float(np.median(ms)), 3),
                   min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3),
                   diagonals_longest=max(T + len(s) for T, s in zip(FRAMES, labels)),
                   workspace_bytes=int(_lib.lib().pk2_transducer_workspace_bytes(_lib.ptr(host), 4, V)),
                   joint_bytes_not_built=int(sum(4 * T * (len(s) + 1) * V for T, s in zip(FRAMES, labels))),
                   loss_sum=float(loss.sum()), status=status.tolist())
        line = json.dumps(out)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
