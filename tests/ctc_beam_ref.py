"""float64 restatement of the CTC prefix beam search contract of DESIGN.md 7.20 on dicts and tuples: the oracle of
tests/test_gpu_ctc_beam.py.  No test logic."""
import math

import numpy as np


def beam_search(logits, blank=0, beam=16, top_tokens=16, lm=None, lm_weight=1.0, insertion_bonus=0.0, lm_ids=None, lm_eos=True):
    """One utterance, logits [T, P] float32.  Returns (nbest, gap, merges): nbest = [(token tuple, score)] best first (ties in
    beam order); gap = the smallest (last kept - first dropped) / last kept over the frames that dropped a candidate (inf
    if none did); merges = the number of extensions that landed on a hypothesis of the beam."""
    x32 = np.asarray(logits, np.float32)
    T, P = x32.shape
    K = min(top_tokens, P - 1)
    x = x32.astype(np.float64)
    y = np.exp(x - x.max(1, keepdims=True))
    y /= y.sum(1, keepdims=True)
    ids = np.arange(P) if lm_ids is None else np.asarray(lm_ids)
    hyps = [((), 1.0, 0.0, lm.start if lm is not None else 0)]      # (prefix, pb, pnb, LM state) in slot order
    expo, gap, merges = 0, math.inf, 0
    for t in range(T):
        order = np.lexsort((np.arange(P), -x32[t]))                 # by logit, ties to the lower column
        cols = [int(c) for c in order if c != blank][:K]
        slot = {l: i for i, (l, _, _, _) in enumerate(hyps)}
        cand = [[l, y[t, blank] * (pb + pnb), y[t, l[-1]] * pnb if l else 0.0, h] for l, pb, pnb, h in hyps]      # the stays
        for l, pb, pnb, h in hyps:
            for c in cols:
                f, hn = 1.0, 0
                if lm is not None:
                    cost, hn = lm.arc(h, int(ids[c]))
                    f = math.exp(-lm_weight * cost + insertion_bonus)
                v = (y[t, c] * f) * (pb + (pnb if not l or c != l[-1] else 0.0))
                if l + (c,) in slot:
                    cand[slot[l + (c,)]][2] += v
                    merges += 1
                else:
                    cand.append([l + (c,), 0.0, v, hn])
        live = sorted((i for i in range(len(cand)) if cand[i][1] + cand[i][2] > 0.0), key=lambda i: -(cand[i][1] + cand[i][2]))
        if not live or not math.isfinite(cand[live[0]][1] + cand[live[0]][2]):
            return [], gap, merges                                  # CTC_NUMERIC
        if len(live) > beam:
            kept, dropped = (cand[live[j]][1] + cand[live[j]][2] for j in (beam - 1, beam))
            gap = min(gap, (kept - dropped) / kept)
        e = math.frexp(cand[live[0]][1] + cand[live[0]][2])[1] - 1  # the best total is in [2^e, 2^(e+1))
        expo += e
        hyps = [(cand[i][0], cand[i][1] * 2.0 ** -e, cand[i][2] * 2.0 ** -e, cand[i][3]) for i in sorted(live[:beam])]
    out = []
    for l, pb, pnb, h in hyps:
        score = math.log(pb + pnb) + expo * math.log(2.0)
        if lm is not None and lm_eos:
            score += -(lm_weight * lm.arc(h, lm.eos_id)[0])
        out.append((l, score))
    return sorted(out, key=lambda a: -a[1]), gap, merges
