"""float64 restatement of the alignment-free LF-MMI numerator: the full-sum forward-backward over an
exported training graph (chain.AlignmentGraphs.export), in the log domain.

  alpha_0(d) = sum_{a: dst=d, src=-1} exp(-w_a + x[0, pdf_a])
  alpha_t(d) = sum_{a: dst=d, src>=0} alpha_{t-1}(src_a) exp(-w_a + x[t, pdf_a])
  log p      = log sum_s alpha_{T-1}(s) exp(-final[s])
  gamma[t,p] = sum_{a: pdf_a=p} P(arc a taken at frame t | x)
"""
import numpy as np


def _scatter_logadd(out, index, values):
    """out[index[i]] = log(exp(out[index[i]]) + exp(values[i])), safely for -inf."""
    if values.size == 0:
        return
    m = np.full(out.shape, -np.inf)
    np.maximum.at(m, index, values)
    m = np.maximum(m, out)
    safe = np.where(np.isfinite(m), m, 0.0)
    acc = np.where(np.isfinite(out), np.exp(out - safe), 0.0)
    np.add.at(acc, index, np.where(np.isfinite(values), np.exp(values - safe[index]), 0.0))
    with np.errstate(divide="ignore"):
        out[:] = np.where(acc > 0, np.log(acc) + safe, -np.inf)


def forward_backward(g, x, with_arcs=False):
    """g: exported graph, x: [T, P] logits (any float type; computed in float64).  Returns (log p, gamma[T, P]) and, with
    with_arcs, the arc occupancies [T, A] as well.  log p = -inf (gamma = 0) when no path of T frames exists."""
    x = np.asarray(x, np.float64)
    T, P = x.shape
    src, dst, pdf = g["src"].astype(np.int64), g["dst"].astype(np.int64), g["pdf"].astype(np.int64)
    w, fin = g["weight"].astype(np.float64), g["final"].astype(np.float64)
    S, A = fin.shape[0], src.shape[0]
    first, rest = np.flatnonzero(src < 0), np.flatnonzero(src >= 0)
    la = np.full((T, S), -np.inf)
    lb = np.full((T, S), -np.inf)
    _scatter_logadd(la[0], dst[first], -w[first] + x[0, pdf[first]])
    for t in range(1, T):
        _scatter_logadd(la[t], dst[rest], la[t - 1, src[rest]] - w[rest] + x[t, pdf[rest]])
    lb[T - 1] = -fin
    for t in range(T - 2, -1, -1):
        _scatter_logadd(lb[t], src[rest], lb[t + 1, dst[rest]] - w[rest] + x[t + 1, pdf[rest]])
    tot = la[T - 1] - fin
    m = tot.max()
    logp = m + np.log(np.exp(tot - m).sum()) if np.isfinite(m) else -np.inf
    # the occupancies [T, A] are kept only when asked for (260 MB for 8000 states over 1700 frames): without them each
    # frame's row is formed, added into gamma and dropped -- the same operations on the same numbers
    occ = np.zeros((T, A)) if with_arcs else None
    gamma = np.zeros((T, P))
    if np.isfinite(logp):
        for t in range(T):
            row = np.zeros(A)
            if t == 0:
                row[first] = np.exp(-w[first] + x[0, pdf[first]] + lb[0, dst[first]] - logp)
            else:
                row[rest] = np.exp(la[t - 1, src[rest]] - w[rest] + x[t, pdf[rest]] + lb[t, dst[rest]] - logp)
            np.add.at(gamma[t], pdf, row)
            if with_arcs:
                occ[t] = row
    return (logp, gamma, occ) if with_arcs else (logp, gamma)


def log_prob_torch(g, x):
    """The same log p as a differentiable float64 torch expression of x[T, P] (probability space: short utterances only)."""
    import torch
    src, dst = torch.from_numpy(g["src"].astype(np.int64)), torch.from_numpy(g["dst"].astype(np.int64))
    pdf = torch.from_numpy(g["pdf"].astype(np.int64))
    w = torch.from_numpy(g["weight"].astype(np.float64))
    efin = torch.from_numpy(np.exp(-g["final"].astype(np.float64)))
    S = efin.shape[0]
    first, rest = torch.nonzero(src < 0).flatten(), torch.nonzero(src >= 0).flatten()
    alpha = torch.zeros(S, dtype=torch.float64).index_add(0, dst[first], torch.exp(-w[first] + x[0, pdf[first]]))
    for t in range(1, x.shape[0]):
        alpha = torch.zeros(S, dtype=torch.float64).index_add(0, dst[rest], alpha[src[rest]] * torch.exp(-w[rest] + x[t, pdf[rest]]))
    return torch.log((alpha * efin).sum())


def enumerate_paths(g, T):
    """Every arc sequence of exactly T frames from the start to a final state, by depth-first search."""
    src, dst, fin = g["src"], g["dst"], g["final"]
    out_arcs = {}
    for k in range(src.shape[0]):
        out_arcs.setdefault(int(src[k]), []).append(k)
    paths, stack = [], []

    def walk(state, t):
        if t == T:
            if np.isfinite(fin[state]):
                paths.append(list(stack))
            return
        for k in out_arcs.get(state, []):
            stack.append(k)
            walk(int(dst[k]), t + 1)
            stack.pop()

    walk(-1, 0)
    return paths
