"""float64 restatement of the transducer beam search contract of DESIGN.md 7.23 on dicts and tuples: the oracle of
tests/test_gpu_transducer_beam.py.  No test logic."""
import math

import numpy as np


def additive(am, table):
    """z(t, prev) of the additive head from float32 am [T, V] and table [V, V]."""
    am, table = np.asarray(am, np.float64), np.asarray(table, np.float64)
    return lambda t, p: am[t] + table[p]


def joiner(enc, pred, w_out, b_out):
    """z(t, prev) = tanh(enc[t] + pred[prev]) w_out^T + b_out from float32 enc [T, J], pred [V, J], w_out [V, J], b_out [V]."""
    enc, pred, w, b = (np.asarray(a, np.float64) for a in (enc, pred, w_out, b_out))
    return lambda t, p: np.tanh(enc[t] + pred[p]) @ w.T + b


def _cut(cand, beam, gap):
    """The `beam` largest of cand [(prefix, score)] in candidate order (ties: the lower candidate), and the gap updated."""
    order = sorted(range(len(cand)), key=lambda i: -cand[i][1])      # stable
    if len(order) > beam:
        gap = min(gap, cand[order[beam - 1]][1] - cand[order[beam]][1])
    return [cand[i] for i in sorted(order[:beam])], gap


def beam_search(z, T, blank=0, beam=4, top_tokens=8, max_symbols=2):
    """One utterance of T frames.  Returns (nbest, gap): nbest = [(token tuple, score)] best first (ties in beam order); gap =
    the smallest difference between the last kept and the first dropped, over the beam cuts (scores) and the token cuts
    (logits) that dropped anything (inf if none did)."""
    A, gap = [((), 0.0)], math.inf
    for t in range(T):
        out = {}                                                     # insertion order = the order the entries were made
        for r in range(max_symbols + 1):
            rows = []
            for h, s in A:
                x = z(t, h[-1] if h else blank)
                lp = x - (x.max() + math.log(np.exp(x - x.max()).sum()))
                rows.append((x, lp))
                out[h] = float(np.logaddexp(out[h], s + lp[blank])) if h in out else s + lp[blank]
            if r == max_symbols:
                break
            cand = []
            for (h, s), (x, lp) in zip(A, rows):
                cols = [int(c) for c in np.lexsort((np.arange(len(x)), -x)) if c != blank]      # ties to the lower column
                K = min(top_tokens, len(cols))
                if len(cols) > K:
                    gap = min(gap, x[cols[K - 1]] - x[cols[K]])
                cand += [(h + (c,), s + lp[c]) for c in cols[:K]]
            A, gap = _cut(cand, beam, gap)
        A, gap = _cut(list(out.items()), beam, gap)
    return sorted(A, key=lambda a: -a[1]), gap
