"""numpy float64 restatement of lattice scoring (pykaldi2_amd/csrc/lattice_score.hip) on the packed lattice
of pykaldi2_amd.score.pack_lattice: arc posteriors, tropical best path, the MBR E-step (Xu, Povey, Mangu, Zhu 2011, as
Kaldi's MinimumBayesRisk, backward pass in gather form, tie rule with tau) and the update loop.  Besides the results it
reports the margins that make a comparison of discrete outputs well defined (distance of every compared difference from
tau, argmax margins, best-path margins)."""
import numpy as np

DELTA = 1e-5
TAU = 1e-9


def arc_costs(P, setting):
    lm, am, wip = (float(x) for x in setting[:3])
    return lm * P.graph.astype(np.float64) + am * P.acoustic.astype(np.float64) + np.where(P.word != 0, wip, 0.0)


def logadd(x, y):
    hi, lo = (x, y) if x >= y else (y, x)
    return hi + np.log1p(np.exp(lo - hi))


def posteriors(P, setting):
    """alpha, arc posteriors, tropical costs v, back-pointers (best incoming arc), best words (global ids), best-path margin."""
    cost = arc_costs(P, setting)
    alpha, v = np.zeros(P.S), np.zeros(P.S)
    bp = np.full(P.S, -1, np.int64)
    margin = np.inf
    for n in range(1, P.S):
        vb, acc = np.inf, 0.0
        cands = []
        for a in range(P.in_off[n], P.in_off[n + 1]):
            x = alpha[P.src[a]] + (-cost[a])
            acc = x if a == P.in_off[n] else logadd(acc, x)
            cand = v[P.src[a]] + cost[a]
            cands.append(cand)
            if cand < vb or bp[n] < 0:
                vb, bp[n] = cand, a
        alpha[n], v[n] = acc, vb
        cs = sorted(cands)
        if len(cs) > 1:
            margin = min(margin, cs[1] - cs[0])
    post = np.exp(alpha[P.src] + (-cost) - alpha[P.dst])
    words, s = [], P.S - 1
    while s > 0:
        a = bp[s]
        if P.word[a] != 0:
            words.append(int(P.word[a]))
        s = P.src[a]
    words.reverse()
    return dict(alpha=alpha, post=post, v=v, backpointer=bp, local_words=words, words=[int(P.word_ids[w]) for w in words],
                cost=float(v[-1]), alpha_end=float(alpha[-1]), margin=margin)


def _rows(Asrc, w, r, cnt):
    """row_a, dec_a and the compared differences for arcs with source rows Asrc (n, Q + 1) and local words w (n,)."""
    n, Q1 = Asrc.shape
    lp = np.where(w != 0, 1.0 + DELTA, 0.0)[:, None]
    a2 = Asrc + lp
    a1 = np.full((n, Q1), np.inf)
    a1[:, 1:] = Asrc[:, :-1] + (w[:, None] != r[None, 1:])
    t = np.minimum(a1, a2)
    m = np.minimum.accumulate(t - cnt[None, :], axis=1)
    a3 = np.full((n, Q1), np.inf)
    a3[:, 1:] = m[:, :-1] + cnt[None, 1:]
    row = np.minimum(t, a3)
    d1 = a1[:, 1:] - np.minimum(a2[:, 1:], a3[:, 1:])
    d2 = a2[:, 1:] - a3[:, 1:]
    dec = np.zeros((n, Q1), np.int8)
    dec[:, 1:] = np.where(d1 <= TAU, 1, np.where(d2 <= TAU, 2, 3))
    compared = np.concatenate([np.abs(d1 - TAU).ravel(), np.abs(d2 - TAU)[d1 > TAU].ravel()])
    return row, dec, (compared.min() if compared.size else np.inf)


def e_step(P, post, hyp):
    """One E-step for the hypothesis `hyp` (local word ids).  Returns risk, gamma (W, Q + 1), and the tie margin."""
    m = len(hyp)
    Q = 2 * m + 1
    r = np.zeros(Q + 1, np.int64)
    r[2:2 * m + 1:2] = hyp
    cnt = np.cumsum(r != 0).astype(np.float64)
    cnt[0] = 0.0
    qi = np.arange(Q + 1)
    A = np.zeros((P.S, Q + 1))
    A[0] = cnt
    dec = np.zeros((P.A, Q + 1), np.int8)
    tie = np.inf
    for lev in range(1, P.depth + 1):
        a0, a1 = P.in_off[P.level_off[lev]], P.in_off[P.level_off[lev + 1]]
        arcs = np.arange(a0, a1)
        row, d, tm = _rows(A[P.src[arcs]], P.word[arcs], r, cnt)
        dec[arcs] = d
        tie = min(tie, tm)
        np.add.at(A, (P.dst[arcs][:, None], qi[None, :]), post[arcs][:, None] * row)
    risk = float(A[P.S - 1, Q])
    B = np.zeros((P.S, Q + 1))
    E = np.zeros((P.S, Q + 1))
    B[P.S - 1, Q] = 1.0
    b = np.zeros((P.A, Q + 1))
    for lev in range(P.depth - 1, -1, -1):
        ks = np.arange(P.out_off[P.level_off[lev]], P.out_off[P.level_off[lev + 1]])
        arcs = P.out_idx[ks]                                   # by source state, ascending arc index within a state
        x = post[arcs][:, None] * B[P.dst[arcs]]
        ba = np.zeros((arcs.size, Q + 1))
        ba[:, Q] = x[:, Q]
        d = dec[arcs]
        for q in range(Q - 1, -1, -1):
            ba[:, q] = x[:, q] + np.where(d[:, q + 1] == 3, ba[:, q + 1], 0.0)
        b[arcs] = ba
        terms = np.zeros((arcs.size, 3, Q + 1))
        terms[:, 0, 1:] = np.where(d[:, 1:] == 2, ba[:, 1:], 0.0)
        terms[:, 1, :Q] = np.where(d[:, 1:] == 1, ba[:, 1:], 0.0)
        terms[:, 2, 0] = ba[:, 0]
        np.add.at(B, (np.broadcast_to(P.src[arcs][:, None, None], terms.shape), np.broadcast_to(qi[None, None, :], terms.shape)), terms)
        e3 = np.zeros((arcs.size, Q + 1))
        e3[:, 1:] = np.where(d[:, 1:] == 3, ba[:, 1:], 0.0)
        np.add.at(E, (P.src[arcs][:, None], qi[None, :]), e3)
    gamma = np.zeros((P.W, Q + 1))
    np.add.at(gamma, (P.word[:, None], qi[None, :]), np.where(dec == 1, b, 0.0))
    esum = np.zeros(Q + 1)
    for s in range(P.S):
        esum += E[s]
    e = np.cumsum(B[0][::-1])[::-1]
    gamma[0] = (gamma[0] + esum) + e
    gamma[:, 0] = 0.0
    return risk, gamma, tie, r


def _top(gamma, q, k):
    """The k best (local word, posterior) of position q: by posterior, ties to the larger word id."""
    order = sorted(range(gamma.shape[0]), key=lambda w: (gamma[w, q], w), reverse=True)
    return [(w, float(gamma[w, q])) for w in order[:k]]


def mbr(P, setting, decode_mbr=True, max_iter=10, bins=0):
    """The record of DESIGN.md 7.13 plus `margins`: dict(sum = max |sum_w gamma - 1| / (Q + 1) over the E-steps, tie,
    argmax, best_path)."""
    pz = posteriors(P, setting)
    hyp = list(pz["local_words"])
    margins = dict(sum=0.0, tie=np.inf, argmax=np.inf, best_path=pz["margin"])
    iters, status = 0, 0
    if 2 * len(hyp) + 1 > P.cap:
        return dict(words=[], conf=np.zeros(0), risk=0.0, iterations=0, status=2, bins=[], margins=margins, post=pz)
    while True:
        risk, gamma, tie, r = e_step(P, pz["post"], hyp)
        Q = r.size - 1
        iters += 1
        margins["tie"] = min(margins["tie"], tie)
        margins["sum"] = max(margins["sum"], float(np.abs(gamma[:, 1:].sum(0) - 1.0).max()) / (Q + 1))
        best = np.zeros(Q + 1, np.int64)
        for q in range(1, Q + 1):
            top = _top(gamma, q, 2)
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
        if 2 * len(new) + 1 > P.cap:
            status = 2
            break
        hyp = new
    out = dict(words=[int(P.word_ids[w]) for w in hyp], conf=np.asarray([gamma[w, 2 * (i + 1)] for i, w in enumerate(hyp)]),
               risk=risk, iterations=iters, status=status, margins=margins, post=pz)
    if bins:
        out["bins"] = [[(int(P.word_ids[w]), v) for w, v in _top(gamma, q, bins)] for q in range(1, Q + 1) if best[q] != 0]
    return out


def edit_distance(x, y):
    """Levenshtein distance with unit costs, the plain DP."""
    prev = list(range(len(y) + 1))
    for i, xi in enumerate(x, 1):
        cur = [i]
        for j, yj in enumerate(y, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (xi != yj)))
        prev = cur
    return prev[-1]


# ---- the lattices the host and the GPU tests share ----
SHAPES = [(1, 1, 2), (2, 1, 2), (3, 2, 3), (8, 4, 5), (20, 8, 8), (33, 5, 4), (40, 12, 10), (70, 6, 5)]
SETTINGS = [(1.0, 1.0 / 7, 0.0), (1.0, 1.0 / 17, 1.0), (1.0, 0.01, 0.5)]


def random_lattice(depth, width, vocab, seed):
    """A layered DAG in the raw compact_lattice form: `depth` levels of `width` states (the last level holds the finals),
    1-2 incoming arcs per state from the previous level, with probability 0.2 one more from two or more levels back; words
    uniform in 1..vocab, epsilon with probability 0.1; every state gets a way forward; one dead-end branch and one
    unreachable state for the packer to trim."""
    rng = np.random.default_rng(seed)
    levels, n = [[0]], 1
    for _ in range(depth):
        levels.append(list(range(n, n + width)))
        n += width
    src, dst = [], []
    for lev in range(1, depth + 1):
        for s in levels[lev]:
            prev = levels[lev - 1]
            for u in rng.choice(len(prev), size=min(len(prev), int(rng.integers(1, 3))), replace=False):
                src.append(prev[int(u)]); dst.append(s)
            if lev >= 2 and rng.random() < 0.2:
                back = levels[int(rng.integers(0, lev - 1))]
                src.append(back[int(rng.integers(0, len(back)))]); dst.append(s)
    for lev in range(0, depth):                      # a way forward for every state
        for s in levels[lev]:
            if s not in src:
                nxt = levels[lev + 1]
                src.append(s); dst.append(nxt[int(rng.integers(0, len(nxt)))])
    dead, unreach = n, n + 1                         # a dead end off the start, and a state nothing reaches
    src += [0, unreach]; dst += [dead, levels[-1][0]]
    n += 2
    A = len(src)
    word = rng.integers(1, vocab + 1, A)
    word[rng.random(A) < 0.1] = 0
    final = np.full(n, np.inf, np.float32)
    final[levels[-1]] = (2.0 * rng.random(len(levels[-1]))).astype(np.float32)
    return dict(num_states=n, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32), word=word.astype(np.int32),
                graph=(4.0 * rng.random(A)).astype(np.float32), acoustic=(40.0 * rng.random(A)).astype(np.float32),
                tid=np.ones(A, np.int32), final=final)


def paths_lattice(paths):
    """Hand-made lattice in the raw compact_lattice form: [(words, probability)], every path its own chain from the start
    state, -log p as the graph cost of its first arc."""
    src, dst, word, graph, finals, n = [], [], [], [], [], 1
    for words, pr in paths:
        s = 0
        for i, w in enumerate(words):
            src.append(s); dst.append(n); word.append(w); graph.append(-np.log(pr) if i == 0 else 0.0)
            s, n = n, n + 1
        finals.append(s)
    final = np.full(n, np.inf, np.float32)
    final[finals] = 0.0
    A = len(src)
    return dict(num_states=n, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                word=np.asarray(word, np.int32), graph=np.asarray(graph, np.float32), acoustic=np.zeros(A, np.float32),
                tid=np.ones(A, np.int32), final=final)
