"""Pruned transducer loss + gradient timing on the frame counts of the LF-MMI bench minibatch (146 / 539 / 569 / 159), seeded
transcripts of one label per 8 frames, a band of S = 5 (a seeded valid band), logits N(0, 2) of shape [4, T, 5, V], V = 43 and
V = 5768:

  pruned_ms   transducer.pruned_loss_and_grad (csrc/transducer_pruned.hip: tp_rows, tp_lattice, tp_grad), events, a warm-up
              call first; median / min / max of --reps.
  torch_ms    the ROW work alone as a user would run it outside HIP: torch.log_softmax over [4, T, 5, V], the gathers of the
              blank and label columns, and autograd's backward of them with given occupancies; the lattice is left out.
  hbm_share   the bytes the call must move, 3 * 4 * sum_n T_n S V (read the logits twice, write the gradient once), over the
              median time, as a share of the 8 TB/s HBM peak.

The three kernels' own times come from the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o tp -- python tools/transducer_pruned_time.py
Prints one JSON line per V; with --out FILE appends them there.  Records, not pass marks."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import _lib, transducer  # noqa: E402

FRAMES, S, HBM = [146, 539, 569, 159], 5, 8.0e12


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, [round(float(f(ms)), 3) for f in (np.median, np.min, np.max)]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev, Tmax = torch.device("cuda"), max(FRAMES)
    for V in (43, 5768):
        rng = np.random.default_rng(V)
        blank = V - 1
        labels = [rng.integers(0, V - 1, size=T // 8).tolist() for T in FRAMES]
        begin = np.zeros((4, Tmax), np.int32)
        for n, (T, lab) in enumerate(zip(FRAMES, labels)):      # a valid band: steps of 0 / 1, clamped to end at U + 1 - S
            Bmax = max(0, len(lab) + 1 - S)
            walk = np.minimum(np.cumsum(rng.random(T) < 1.5 * Bmax / T), Bmax)
            begin[n, :T] = np.maximum(walk - walk[0], Bmax - (S - 1) * (T - 1 - np.arange(T)))
        begin = torch.from_numpy(begin).to(dev)
        z = torch.from_numpy(rng.normal(0, 2, size=(4, Tmax, S, V)).astype(np.float32)).to(dev)
        (loss, _, status), pruned = _events(lambda: transducer.pruned_loss_and_grad(z, begin, FRAMES, labels, blank), reps)
        # the row work in torch: forward and backward of log_softmax + gathers, occupancies given
        u = (begin.long()[:, :, None] + torch.arange(S, device=dev)).clamp(max=max(map(len, labels)) - 1)
        lab = torch.zeros((4, max(map(len, labels))), dtype=torch.long, device=dev)
        for n, seq in enumerate(labels):
            lab[n, :len(seq)] = torch.tensor(seq, device=dev)
        col = torch.gather(lab, 1, u.reshape(4, -1)).reshape(4, Tmax, S, 1)
        occ = torch.rand((2, 4, Tmax, S), device=dev)
        zt = z.clone().requires_grad_()

        def row_work():
            zt.grad = None
            logy = torch.log_softmax(zt, -1)
            (logy[..., blank] * occ[0] + torch.gather(logy, 3, col)[..., 0] * occ[1]).sum().backward()
            return zt.grad

        _, torch_ms = _events(row_work, reps)
        must_move = 3 * 4 * sum(FRAMES) * S * V
        out = dict(frames=FRAMES, V=V, S=S, labels=[len(s) for s in labels], reps=reps, pruned_ms=pruned, torch_row_work_ms=torch_ms,
                   bytes_must_move=must_move, hbm_share=round(must_move / (pruned[0] * 1e-3) / HBM, 4),
                   workspace_bytes=int(_lib.lib().pk2_transducer_pruned_workspace_bytes(4, Tmax, S, V)),
                   diagonals_longest=max(T + len(s) for T, s in zip(FRAMES, labels)), loss_sum=float(loss.sum()), status=status.tolist())
        line = json.dumps(out)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
