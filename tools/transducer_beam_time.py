"""Transducer beam search timing on the subsampled frame counts of the bench minibatch (49 / 180 / 190 / 53), R = 2 labels per
frame, top_tokens = 8, V = 72 and V = 512, beam 4 / 8 / 32, the additive head and a joiner of width J = 256:

  call    transducer.beam_search_raw: tb_search (csrc/transducer_beam.hip), one launch, no copy to the host,
  torch   the same (R + 1) joint evaluations per frame as batched torch ops over [N, beam] rows, frame after frame: (tanh,
          matmul,) add, log_softmax, topk.  No search logic, no bookkeeping: what a user has without the kernel, at its cheapest.

Events, alternating, a warm-up call each first; median / min / max of --reps (default 20).  us_per_frame is the time over 190,
the frames of the longest utterance, whose workgroup ends last.  Prints one JSON line per configuration; with --out FILE
appends them there."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import transducer  # noqa: E402

FRAMES = [49, 180, 190, 53]
R, K, J = 2, 8, 256


def torch_steps(x, rows, joiner, beam):
    """(R + 1) joint evaluations per frame for [N, beam] hypotheses whose last token is a fixed column: the arithmetic only."""
    N, T, _ = x.shape
    prev = torch.arange(N * beam, device=x.device).reshape(N, beam) % rows.shape[0]
    pr = rows[prev]                                                  # [N, beam, D]
    keep = None
    for t in range(T):
        for _ in range(R + 1):
            s = x[:, t, None, :] + pr
            z = torch.tanh(s) @ joiner[0].t() + joiner[1] if joiner else s
            keep = torch.log_softmax(z, dim=2).topk(K, dim=2)
    return keep


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    for V in (72, 512):
        rng = np.random.default_rng(V)
        blank = V - 1
        f = lambda *shape, scale=1.0: torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(dev)
        am, table = f(4, max(FRAMES), V, scale=2.0), f(V, V)
        am[:, :, blank] += 3.0
        enc, pred, w, b = f(4, max(FRAMES), J), f(V, J), f(V, J, scale=3.0 / J ** 0.5), f(V, scale=0.5)
        b[blank] += 3.0
        for form, (x, rows, joiner) in (("additive", (am, table, None)), ("joiner", (enc, pred, (w, b)))):
            for beam in (4, 8, 32):
                fns = dict(call=lambda: transducer.beam_search_raw(x, FRAMES, rows, blank, beam, K, R, joiner),
                           torch=lambda: torch_steps(x, rows, joiner, beam))
                ms = {k: [] for k in fns}
                for fn in fns.values():
                    fn()
                torch.cuda.synchronize()
                for _ in range(reps):
                    for k, fn in fns.items():
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn()
                        e.record()
                        torch.cuda.synchronize()
                        ms[k].append(a.elapsed_time(e))
                out = dict(frames=FRAMES, V=V, form=form, J=J if joiner else 0, beam=beam, top_tokens=K, max_symbols=R, reps=reps)
                for k, v in ms.items():
                    out[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3), max_ms=round(float(np.max(v)), 3),
                                  us_per_frame=round(1e3 * float(np.median(v)) / max(FRAMES), 2))
                tokens, lens, scores, status = fns["call"]()
                out["best_len"], out["best_score"], out["status"] = lens[:, 0].tolist(), scores[:, 0].tolist(), status.tolist()
                line = json.dumps(out)
                print(line, flush=True)
                if out_path:
                    with open(out_path, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
