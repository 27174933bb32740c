"""numpy float64 restatements of MBR system combination (pykaldi2_amd/csrc/lattice_combine.hip), both on top
of mbr_ref.posteriors and mbr_ref.e_step:

  combine(Ps, weights, setting)        (a) the rule the kernels implement: one E-step per system on its own lattice, the
                                       statistics added with the normalised weights in ascending system order
  union_mbr(Ps, weights, setting)      (b) mbr_ref.mbr on the explicit union lattice: the systems' start states merged, the
                                       normaliser Z_k - log wn_k added to every final arc of system k in float64

(b) is the definition -- lattice-combine followed by lattice-mbr-decode -- and (a) must agree with it; a union that adds an
exit state per system with one more epsilon arc does not (same risk, other confidences: the extra arc changes where the
tie rule puts deletions) and is not an oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import score  # noqa: E402


def case(seed):
    """The lattices (raw dicts) and weights of generator case `seed`; the draw order is part of the definition."""
    rng = np.random.default_rng(seed)
    K = int(rng.integers(2, 4))
    depth, width, vocab = R.SHAPES[seed % 8]
    lats = []
    for k in range(K):
        lats.append(R.random_lattice(max(1, depth + int(rng.integers(-1, 2))), width, vocab, 1000 * seed + k))
    weights = rng.random(K) + 0.2
    return lats, weights


def normalised(weights):
    w = np.asarray(weights, np.float64).reshape(-1)
    wn = w / w.sum()
    return wn, np.log(wn)


def combine(Ps, weights, setting, decode_mbr=True, max_iter=10, bins=0):
    """(a).  The record of CombinedBatch.mbr plus `margins`: sum, tie and argmax as in mbr_ref.mbr over all systems and
    E-steps (sum also over Gamma), best_path = min(the starting system's best-path margin, the gap between the two
    smallest v_k + Z_k - log wn_k)."""
    H = score.pack_groups([Ps], [weights])
    wn, lw, vocab, maps = H["wn"], H["log_wn"], H["vocab"][0], H["maps"]
    K, cap = len(Ps), H["cap"][0]
    pz = [R.posteriors(P, setting) for P in Ps]
    start = [(pz[k]["cost"] + pz[k]["alpha_end"]) - lw[k] for k in range(K)]
    ks = 0
    for k in range(1, K):
        if start[k] < start[ks]:
            ks = k
    gap = np.inf if K == 1 else float(np.diff(np.sort(start))[0])
    margins = dict(sum=0.0, tie=np.inf, argmax=np.inf, best_path=min(pz[ks]["margin"], gap))
    hyp = [int(x) for x in np.searchsorted(vocab, pz[ks]["words"])]
    iters, status = 0, 0
    if 2 * len(hyp) + 1 > cap:
        return dict(words=[], conf=np.zeros(0), risk=0.0, iterations=0, status=2, system=ks, bins=[], margins=margins)
    while True:
        Q = 2 * len(hyp) + 1
        Gamma, risk = np.zeros((vocab.size, Q + 1)), 0.0
        for k, P in enumerate(Ps):
            risk_k, gamma_k, tie, r_k = R.e_step(P, pz[k]["post"], [int(maps[k][x]) for x in hyp])
            margins["tie"] = min(margins["tie"], tie)
            margins["sum"] = max(margins["sum"], float(np.abs(gamma_k[:, 1:].sum(0) - 1.0).max()) / (Q + 1))
            have = np.flatnonzero(maps[k] < P.W)
            Gamma[have] += wn[k] * gamma_k[maps[k][have]]
            risk += wn[k] * risk_k
        iters += 1
        margins["sum"] = max(margins["sum"], float(np.abs(Gamma[:, 1:].sum(0) - 1.0).max()) / (Q + 1))
        r = np.zeros(Q + 1, np.int64)
        r[2:2 * len(hyp) + 1:2] = hyp
        best = np.zeros(Q + 1, np.int64)
        for q in range(1, Q + 1):
            top = R._top(Gamma, q, 2)
            best[q] = top[0][0]
            if len(top) > 1:
                margins["argmax"] = min(margins["argmax"], top[0][1] - top[1][1])
        new = [int(w) for w in best[1:] if w != 0]
        if not decode_mbr or np.array_equal(best[1:], r[1:]):
            status = 0
            break
        if iters >= max_iter:
            status = 1
            break
        if 2 * len(new) + 1 > cap:
            status = 2
            break
        hyp = new
    out = dict(words=[int(vocab[w]) for w in hyp], conf=np.asarray([Gamma[w, 2 * (i + 1)] for i, w in enumerate(hyp)]),
               risk=risk, iterations=iters, status=status, system=ks, margins=margins)
    if bins:
        out["bins"] = [[(int(vocab[w]), v) for w, v in R._top(Gamma, q, bins)] for q in range(1, Q + 1) if best[q] != 0]
    return out


def union_lattice(Ps, weights, setting):
    """(b)'s lattice, packed, with the whole float64 arc cost in .graph (score it with the setting (1, 0, 0): 1 x + 0 y + 0
    is exact): the start states merged, every other state of every system its own, the arcs into a system's end state
    turned back into final weights that carry cost + Z_k - log wn_k."""
    wn, lw = normalised(weights)
    src, dst, word, cost, fin_state, fin_cost, n = [], [], [], [], [], [], 1
    for k, P in enumerate(Ps):
        z = R.posteriors(P, setting)
        c = R.arc_costs(P, setting)
        new = np.concatenate([[0], n + np.arange(P.S - 2), [-1]]).astype(np.int64)     # start merged, the end state dropped
        n += P.S - 2
        for a in range(P.A):
            if P.dst[a] == P.S - 1:
                assert P.word[a] == 0 and P.src[a] != 0, "a final start state cannot be merged"
                fin_state.append(int(new[P.src[a]])); fin_cost.append(c[a] + (z["alpha_end"] - lw[k]))
            else:
                src.append(int(new[P.src[a]])); dst.append(int(new[P.dst[a]])); word.append(int(P.word_ids[P.word[a]]))
                cost.append(c[a])
    assert len(set(fin_state)) == len(fin_state)
    final = np.full(n, np.inf, np.float32)
    final[fin_state] = 0.0
    A = len(src)
    lat = dict(num_states=n, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32), word=np.asarray(word, np.int32),
               graph=np.zeros(A, np.float32), acoustic=np.zeros(A, np.float32), final=final)
    U = score.pack_lattice(lat, "union")
    fc = np.full(n, np.nan)
    fc[fin_state] = fin_cost
    both = np.concatenate([np.asarray(cost, np.float64), fc[np.flatnonzero(np.isfinite(final))]])
    U.graph = both[U.orig_arc]
    U.acoustic = np.zeros(U.A)
    assert np.isfinite(U.graph).all()
    return U


def union_mbr(Ps, weights, setting, **kw):
    """(b): mbr_ref.mbr of the explicit union lattice."""
    return R.mbr(union_lattice(Ps, weights, setting), (1.0, 0.0, 0.0), **kw)
