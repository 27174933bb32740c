"""CTC loss + gradient timing on the frame counts of the LF-MMI bench minibatch (146 / 539 / 569 / 159), P = 42 and P = 5768,
seeded transcripts of about one label per 8 frames, logits N(0, 2):

  ours   ctc.ctc_loss_and_grad on the unnormalised logits (csrc/ctc.hip: three launches),
  torch  log_softmax + torch.nn.functional.ctc_loss (reduction='sum') + backward to the logits, same device, same job.

Both are timed with events, alternating, a warm-up call each first; median / min / max of --reps.  The per-launch kernel times
(ctc_rows, ctc_chains, ctc_grad: the per-frame time of ctc_chains is its time over the longest utterance's frames) come
from the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o ctc -- python tools/ctc_time.py --ours-only
Prints one JSON line per P; with --out FILE appends them there."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import ctc  # noqa: E402

FRAMES = [146, 539, 569, 159]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    ours_only = "--ours-only" in sys.argv
    dev = torch.device("cuda")
    for P in (42, 5768):
        rng = np.random.default_rng(P)
        blank = P - 1
        labels = [rng.integers(0, P - 1, size=T // 8).tolist() for T in FRAMES]
        x = torch.from_numpy(rng.normal(0, 2, size=(4, max(FRAMES), P)).astype(np.float32)).to(dev)
        tgt = torch.tensor([lab + [0] * (max(map(len, labels)) - len(lab)) for lab in labels], device=dev)
        tl, il = torch.tensor([len(s) for s in labels]), torch.tensor(FRAMES)

        def ours():
            return ctc.ctc_loss_and_grad(x, FRAMES, labels, blank)

        def theirs():
            xr = x.detach().requires_grad_(True)
            loss = torch.nn.functional.ctc_loss(xr.log_softmax(2).transpose(0, 1), tgt, il, tl, blank=blank, reduction="sum")
            loss.backward()
            return loss, xr.grad

        fns = dict(ours=ours) if ours_only else dict(ours=ours, torch=theirs)
        ms = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        out = dict(frames=FRAMES, P=P, labels=[len(s) for s in labels], reps=reps)
        for k, v in ms.items():
            out[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3), max_ms=round(float(np.max(v)), 3))
        if not ours_only:
            lo, go, _ = ours()
            lt, gt = theirs()
            out["ratio_torch_over_ours"] = round(out["torch"]["median_ms"] / out["ours"]["median_ms"], 3)
            out["loss_sum"] = [float(lo.sum()), float(lt)]
            out["grad_max_abs_diff"] = max(float((go[n, :T] - gt[n, :T]).abs().max()) for n, T in enumerate(FRAMES))
        line = json.dumps(out)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
