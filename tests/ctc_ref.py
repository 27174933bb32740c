"""float64 log-domain restatement of the CTC contract of DESIGN.md 7.19, vectorised over the states: the oracle of
tests/test_ctc_host.py (which pins it against an enumeration and against torch) and tests/test_gpu_ctc.py."""
import numpy as np


def _lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))


def loss_and_grad(logits, labels, blank=0, weight=1.0):
    """(loss, grad [T, P], status) of one utterance: logits [T, P] unnormalised, labels without the blank.
    status 2 (loss 0, grad 0) when T < max(1, L + number of i with l_i = l_{i+1})."""
    x = np.asarray(logits, np.float64)
    T, P = x.shape
    lab = np.asarray(labels, np.int64).reshape(-1)
    L, S = len(lab), 2 * len(lab) + 1
    if T < max(1, L + int((lab[1:] == lab[:-1]).sum())):
        return 0.0, np.zeros((T, P)), 2
    m = x.max(1, keepdims=True)
    logy = x - (m + np.log(np.exp(x - m).sum(1, keepdims=True)))
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S + 2, bool)                  # state s may be entered from s - 2 (and s + 2 from s); two pads behind
    skip[3:S:2] = lab[1:] != lab[:-1]
    # state s lives in column s + 2: two columns of -inf on either side stand for the states that do not exist.  A frame
    # updates only its band: the states that can be reached from the start and can still reach the end (the rest is -inf).
    band = lambda t: (max(0, S - 2 * (T - t)), min(S, 2 * t + 2))      # noqa: E731
    la = np.full((T, S + 4), -np.inf)
    la[0, 2:4] = np.append(logy[0, ext[:2]], -np.inf)[:2]
    for t in range(1, T):
        lo, hi = band(t)
        p = la[t - 1]
        la[t, lo + 2:hi + 2] = logy[t, ext[lo:hi]] + _lse3(p[lo + 2:hi + 2], p[lo + 1:hi + 1], np.where(skip[lo:hi], p[lo:hi], -np.inf))
    logp = np.logaddexp.reduce(la[T - 1, 2:S + 2][-2:])
    grad = np.exp(logy)
    q = np.full(S + 4, -np.inf)                   # beta of the frame behind, with the emission of its own frame (the contract's)
    for t in range(T - 1, -1, -1):
        lo, hi = band(t)
        b = np.full(S + 4, -np.inf)
        if t == T - 1:
            b[S:S + 2] = np.append(-np.inf, logy[t, ext[-2:]])[-2:]
        else:
            b[lo + 2:hi + 2] = logy[t, ext[lo:hi]] + _lse3(q[lo + 2:hi + 2], q[lo + 3:hi + 3],
                                                           np.where(skip[lo + 2:hi + 2], q[lo + 4:hi + 4], -np.inf))
        occ = np.exp(la[t, lo + 2:hi + 2] + b[lo + 2:hi + 2] - logy[t, ext[lo:hi]] - logp)      # P(state s at frame t)
        grad[t] -= np.bincount(ext[lo:hi], weights=occ, minlength=P)
        q = b
    return -logp, weight * grad, 0
