"""float64 restatement of the transducer contract of DESIGN.md 7.21 with the 4-D joint built EXPLICITLY: the oracle of
tests/test_transducer_host.py (which pins it against an enumeration and central differences) and tests/test_gpu_transducer.py."""
import numpy as np


def lattice(am, lm, labels, blank=0):
    """(log p, logy [T, U+1, V], py, px [T, U+1], alpha, beta [T+1, U+2] padded with -inf) of one utterance."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    lab = np.asarray(labels, np.int64).reshape(-1)
    T, U = am.shape[0], len(lab)
    z = am[:, None, :] + lm[None, :U + 1, :]
    m = z.max(2, keepdims=True)
    logy = z - (m + np.log(np.exp(z - m).sum(2, keepdims=True)))
    py = logy[:, :, blank]
    px = np.full((T, U + 1), -np.inf)
    px[:, :U] = logy[:, np.arange(U), lab]
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
    return alpha[T - 1, U] + py[T - 1, U], logy, py, px, alpha, beta


def loss_and_grad(am, lm, labels, blank=0, weight=1.0):
    """(loss, grad_am [T, V], grad_lm [U+1, V]) of one utterance: am [T, V], lm [>= U+1, V] unnormalised."""
    lab = np.asarray(labels, np.int64).reshape(-1)
    logp, logy, py, px, alpha, beta = lattice(am, lm, lab, blank)
    T, U1, V = logy.shape
    occ_y = np.exp(alpha[:T, :U1] + py + beta[1:, :U1] - logp)
    occ_x = np.exp(alpha[:T, :U1] + px + beta[:T, 1:] - logp)
    g = (occ_x + occ_y)[:, :, None] * np.exp(logy)      # d(-log p) / dz[t, u, .]
    g[:, :, blank] -= occ_y
    g[:, np.arange(U1 - 1), lab] -= occ_x[:, :U1 - 1]
    return -logp, weight * g.sum(1), weight * g.sum(0)


def normaliser_f32(am, lm):
    """The factorised normaliser S[t, u] = sum_v exp(am - max am) exp(lm - max lm) as float32 arithmetic forms it."""
    ea = np.exp((am - am.max(1, keepdims=True)).astype(np.float32)).astype(np.float32)
    el = np.exp((lm - lm.max(1, keepdims=True)).astype(np.float32)).astype(np.float32)
    return (ea[:, None, :] * el[None, :, :]).sum(2, dtype=np.float32)


def greedy(am, table, blank=0, max_symbols=8):
    """Greedy decoding with a table predictor: float32 sums, np.argmax takes the lower column of a tie."""
    am, table = np.asarray(am, np.float32), np.asarray(table, np.float32)
    out, prev = [], blank
    for t in range(am.shape[0]):
        for _ in range(max_symbols):
            v = int(np.argmax(am[t] + table[prev]))
            if v == blank:
                break
            out.append(v)
            prev = v
    return out
