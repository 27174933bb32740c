"""CTC prefix beam search timing on the frame counts of the LF-MMI bench minibatch (146 / 539 / 569 / 159), logits N(0, 2) with
+3 on the blank (the last column), P = 42 and P = 5768, (beam, top_tokens) = (16, 16) and (128, 32), without an LM and with a
seeded trigram LM over the tokens (unigrams, 8 bigrams per token, 4 trigrams per bigram):

  call    ctc.beam_search_raw: ctcb_rows + ctcb_search (csrc/ctc_beam.hip), no copy to the host,
  greedy  ctc.greedy_decode (torch ops and a copy to the host), for scale.

Events, alternating, a warm-up call each first; median / min / max of --reps (default 30).  call_us_per_frame is the call
over 569, the frames of the longest utterance, whose workgroup ends last: the search's time per frame with ctcb_rows still
in it.  ctc_chains' 1.13 us per frame (profiles/ctc_time.txt) is the scale of a per-frame chain with one barrier.  Prints one
JSON line per configuration (--config I: only the I-th of the eight); with --out FILE appends them there.  The split into
ctcb_rows and ctcb_search comes from the profiler, one configuration in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o beam -- python tools/ctc_beam_time.py --reps 20 --config 0"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import ctc, ngram  # noqa: E402

FRAMES = [146, 539, 569, 159]
CTC_CHAINS_US_PER_FRAME = 1.13      # profiles/ctc_time.txt


def trigram(P, rng):
    """Words 1..P-1 are the tokens (column c -> word c + 1), <s> = P, </s> = P + 1."""
    toks = np.arange(1, P)
    grams = {(int(w),): (-rng.uniform(0.5, 3.0), -rng.uniform(0.0, 0.5)) for w in range(1, P + 2)}
    for a in toks.tolist() + [P]:
        for b in rng.choice(toks, size=min(8, P - 1), replace=False).tolist():
            grams[(a, b)] = (-rng.uniform(0.1, 2.0), -rng.uniform(0.0, 0.5))
            for c in rng.choice(toks, size=min(4, P - 1), replace=False).tolist():
                grams[(a, b, c)] = (-rng.uniform(0.1, 2.0), None)
    return ngram.NgramLM.from_ngrams(grams, P, P + 1, 3)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    only = int(sys.argv[sys.argv.index("--config") + 1]) if "--config" in sys.argv else None
    dev = torch.device("cuda")
    index = -1
    for P in (42, 5768):
        rng = np.random.default_rng(P)
        blank = P - 1
        x = rng.normal(0, 2, size=(4, max(FRAMES), P)).astype(np.float32)
        x[:, :, blank] += 3.0
        x = torch.from_numpy(x).to(dev)
        lm = trigram(P, rng)
        ids = np.arange(1, P + 1)
        for beam, K in ((16, 16), (128, 32)):
            for with_lm in (False, True):
                index += 1
                if only is not None and index != only:
                    continue
                kw = dict(lm=lm, lm_ids=ids, lm_weight=0.5) if with_lm else {}
                fns = dict(call=lambda: ctc.beam_search_raw(x, FRAMES, blank, beam, K, **kw),
                           greedy=lambda: ctc.greedy_decode(x, FRAMES, blank))
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
                out = dict(frames=FRAMES, P=P, beam=beam, top_tokens=K, lm=with_lm, reps=reps)
                for k, v in ms.items():
                    out[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3), max_ms=round(float(np.max(v)), 3))
                out["call_us_per_frame"] = round(1e3 * out["call"]["median_ms"] / max(FRAMES), 2)
                out["ctc_chains_us_per_frame"] = CTC_CHAINS_US_PER_FRAME
                tokens, lens, scores, status = fns["call"]()
                out["best_len"], out["best_score"], out["status"] = lens[:, 0].tolist(), scores[:, 0].tolist(), status.tolist()
                line = json.dumps(out)
                print(line, flush=True)
                if out_path:
                    with open(out_path, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
