"""float64 restatement of the pruned transducer contract of DESIGN.md 7.22: the pruning ranges, the loss on the 4-D logits of
a band, and the banded join with its two gradients.  tests/test_transducer_pruned_host.py pins it against
tests/transducer_ref.py and central differences; tests/test_gpu_transducer_pruned.py uses it as the oracle."""
import numpy as np


def ranges(gamma, T, U, S):
    """begin [T] of one utterance from gamma [>= T, >= U + 1]: the five lines of the contract."""
    g = np.asarray(gamma, np.float64)
    Bmax = max(0, U + 1 - S)
    raw = np.empty(T, np.int64)
    for t in range(T):
        win = [sum(float(g[t, u]) for u in range(s, min(s + S - 1, U) + 1)) for s in range(Bmax + 1)]      # ascending u
        raw[t] = np.clip(int(np.argmax(win)), max(0, Bmax - (S - 1) * (T - 1 - t)), min(Bmax, (S - 1) * t))
    b = np.minimum.accumulate(raw[::-1])[::-1]
    begin = b.copy()
    for t in range(T - 2, -1, -1):
        begin[t] = max(b[t], begin[t + 1] - (S - 1))
    return begin


def pruned_loss_and_grad(logits, begin, labels, blank=0, weight=1.0):
    """(loss, grad [T, S, V]) of one utterance: logits [T, S, V] unnormalised, row (t, s) the cell u = begin[t] + s."""
    z = np.asarray(logits, np.float64)
    lab = np.asarray(labels, np.int64).reshape(-1)
    T, S, V = z.shape
    U = len(lab)
    m = z.max(2, keepdims=True)
    logy = z - (m + np.log(np.exp(z - m).sum(2, keepdims=True)))
    py, px = np.full((T, U + 2), -np.inf), np.full((T, U + 2), -np.inf)
    for t in range(T):
        for s in range(S):
            u = int(begin[t]) + s
            if u <= U:
                py[t, u] = logy[t, s, blank]
                if u < U:
                    px[t, u] = logy[t, s, lab[u]]
    alpha = np.full((T + 1, U + 2), -np.inf)
    for t in range(T):
        for u in range(U + 1):
            alpha[t, u] = 0.0 if t == u == 0 else np.logaddexp(alpha[t - 1, u] + py[t - 1, u] if t else -np.inf,
                                                                alpha[t, u - 1] + px[t, u - 1] if u else -np.inf)
    beta = np.full((T + 1, U + 2), -np.inf)
    beta[T, U] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            beta[t, u] = np.logaddexp(py[t, u] + beta[t + 1, u], px[t, u] + beta[t, u + 1])
    logp = alpha[T - 1, U] + py[T - 1, U]
    grad = np.zeros_like(z)
    for t in range(T):
        for s in range(S):
            u = int(begin[t]) + s
            if u > U:
                continue
            oy = np.exp(alpha[t, u] + py[t, u] + beta[t + 1, u] - logp)
            ox = np.exp(alpha[t, u] + px[t, u] + beta[t, u + 1] - logp) if u < U else 0.0
            grad[t, s] = (ox + oy) * np.exp(logy[t, s])
            grad[t, s, blank] -= oy
            if u < U:
                grad[t, s, lab[u]] -= ox
    return -logp, weight * grad


def join(enc, pred, begin, T, U, S, tanh=True, dh=None):
    """h [Tpad, S, J] = tanh(enc[t] + pred[begin[t] + s]) (zeros for t >= T, u > U) and, with dh, (h, d_enc, d_pred)."""
    enc, pred = np.asarray(enc, np.float64), np.asarray(pred, np.float64)
    h = np.zeros((enc.shape[0], S, enc.shape[1]))
    d_enc, d_pred = np.zeros_like(enc), np.zeros_like(pred)
    for t in range(T):
        for s in range(S):
            u = int(begin[t]) + s
            if u <= U:
                x = enc[t] + pred[u]
                h[t, s] = np.tanh(x) if tanh else x
                if dh is not None:
                    g = np.asarray(dh[t, s], np.float64) * (1.0 - h[t, s] ** 2 if tanh else 1.0)
                    d_enc[t] += g
                    d_pred[u] += g
    return h if dh is None else (h, d_enc, d_pred)
