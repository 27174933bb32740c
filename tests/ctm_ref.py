"""numpy float64 restatement of the word times of lattice scoring (ws_times_kernel in
pykaldi2_amd/csrc/lattice_score.hip) on top of tests/mbr_ref.py: state times from the lengths of the transition-id strings,
the time statistics TB / TE of the last E-step (Xu et al., Appendix C, tau_b / tau_e in this project's gather form), the
best path's own arc times, and `timed`, which gives any lattice of mbr_ref's makers consistent string lengths."""
import numpy as np

import mbr_ref as R


def arc_lengths(P, lat):
    """Length of the transition-id string of every PACKED arc, arc by arc (the finals' strings on the arcs packing made of
    them); None for a form without strings."""
    if "arcs" in lat and "finals" in lat:
        al = [len(a[4][2]) for a in lat["arcs"]]
        fl = [len(f[2]) for f in lat["finals"]]
        fin = [s for s, f in enumerate(lat["finals"]) if np.isfinite(f[0])]
    else:
        n = int(lat["num_states"])
        fin = [s for s in range(n) if np.isfinite(lat["final"][s])]
        if "tid_off" in lat:
            al = [int(lat["tid_off"][a + 1] - lat["tid_off"][a]) for a in range(len(lat["src"]))]
            fl = [int(lat["final_tid_off"][s + 1] - lat["final_tid_off"][s]) for s in range(n)]
        elif "tid" in lat:
            al, fl = [int(x > 0) for x in lat["tid"]], [0] * n
        else:
            return None
    nA = len(al)
    return np.asarray([al[k] if k < nA else fl[fin[k - nA]] for k in P.orig_arc], np.int64)


def state_times(P, lat):
    """t(0) = 0, t(n) = t(s_a) + len_a, the same over all incoming arcs of n (ValueError otherwise) except for the end state,
    which takes the maximum."""
    lens = arc_lengths(P, lat)
    if lens is None:
        raise ValueError("no strings")
    t = np.full(P.S, -1, np.int64)
    t[0] = 0
    for a in range(P.A):                                   # sorted by destination: the sources are final here
        n, x = int(P.dst[a]), int(t[P.src[a]] + lens[a])
        if t[n] >= 0 and t[n] != x and n != P.S - 1:
            raise ValueError("state %d: %d and %d" % (n, t[n], x))
        t[n] = max(t[n], x)
    return t


def e_step_times(P, post, hyp, t):
    """The E-step of mbr_ref.e_step for `hyp` (local words) with its arc quantities kept: returns gamma (W, Q + 1), TB, TE
    (W, Q + 1; row 0 is not computed) and G1 = sum over a word's arcs of [dec = 1] b_a(q), which must reproduce gamma."""
    risk, gamma, tie, r = R.e_step(P, post, hyp)
    Q = r.size - 1
    cnt = np.cumsum(r != 0).astype(np.float64)
    cnt[0] = 0.0
    qi = np.arange(Q + 1)
    A = np.zeros((P.S, Q + 1))
    A[0] = cnt
    dec = np.zeros((P.A, Q + 1), np.int8)
    for lev in range(1, P.depth + 1):
        arcs = np.arange(P.in_off[P.level_off[lev]], P.in_off[P.level_off[lev + 1]])
        row, d, _ = R._rows(A[P.src[arcs]], P.word[arcs], r, cnt)
        dec[arcs] = d
        np.add.at(A, (P.dst[arcs][:, None], qi[None, :]), post[arcs][:, None] * row)
    B = np.zeros((P.S, Q + 1))
    B[P.S - 1, Q] = 1.0
    b = np.zeros((P.A, Q + 1))
    for lev in range(P.depth - 1, -1, -1):
        arcs = P.out_idx[np.arange(P.out_off[P.level_off[lev]], P.out_off[P.level_off[lev + 1]])]
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
    TB, TE, G1 = np.zeros((P.W, Q + 1)), np.zeros((P.W, Q + 1)), np.zeros((P.W, Q + 1))
    hit = np.where(dec == 1, b, 0.0)                     # np.add.at adds in arc order: ascending within a word
    idx = (P.word[:, None], qi[None, :])
    np.add.at(TB, idx, t[P.src].astype(np.float64)[:, None] * hit)
    np.add.at(TE, idx, t[P.dst].astype(np.float64)[:, None] * hit)
    np.add.at(G1, idx, hit)
    for m_ in (TB, TE, G1):
        m_[:, 0] = 0.0
    return dict(gamma=gamma, TB=TB, TE=TE, G1=G1, r=r)


def _pair(s, w, q):
    g = s["gamma"][w, q]
    if w == 0 or g <= 0:
        return (-1.0, -1.0), g
    return (s["TB"][w, q] / g, s["TE"][w, q] / g), g


def mbr_times(P, setting, t, decode_mbr=True, max_iter=10, bins=0):
    """The record of mbr_ref.mbr plus times (m, 2), path_times (m0, 2) and with bins bin_times, and next to them the
    posteriors the times were divided by (time_gamma, bin_gamma) for the tolerance and `stats` (e_step_times of the last
    E-step; None when no E-step ran)."""
    t = np.asarray(t, np.int64)
    out = R.mbr(P, setting, decode_mbr=decode_mbr, max_iter=max_iter, bins=bins)
    pz = out["post"]
    path, s = [], P.S - 1
    while s > 0:
        a = pz["backpointer"][s]
        if P.word[a] != 0:
            path.append((t[P.src[a]], t[P.dst[a]]))
        s = P.src[a]
    out["path_times"] = np.asarray(path[::-1], np.int32).reshape(-1, 2)
    out["times"], out["time_gamma"], out["stats"] = np.zeros((0, 2)), np.zeros(0), None
    if bins:
        out["bin_times"], out["bin_gamma"] = [], []
    if out["iterations"] == 0:
        return out
    hyp = [int(np.searchsorted(P.word_ids, w)) for w in out["words"]]
    s = out["stats"] = e_step_times(P, pz["post"], hyp, t)
    pairs = [_pair(s, w, 2 * (i + 1)) for i, w in enumerate(hyp)]
    out["times"] = np.asarray([p[0] for p in pairs], np.float64).reshape(-1, 2)
    out["time_gamma"] = np.asarray([p[1] for p in pairs], np.float64)
    if bins:
        Q = s["r"].size - 1
        for q in range(1, Q + 1):
            top = R._top(s["gamma"], q, bins)
            if top[0][0] != 0:
                ps = [_pair(s, w, q) for w, _ in top]
                out["bin_times"].append([p[0] for p in ps])
                out["bin_gamma"].append([p[1] for p in ps])
        assert [[w for w, _ in bn] for bn in out["bins"]] == \
            [[int(P.word_ids[w]) for w, _ in R._top(s["gamma"], q, bins)] for q in range(1, Q + 1) if R._top(s["gamma"], q, 1)[0][0] != 0]
    return out


def timed(lat, seed, step=10, jitter=6):
    """`lat` (raw compact_lattice form of mbr_ref's makers) in the tid_off form with consistent string lengths: a state of
    level L (longest arc count from the start) is reached at frame step L + U{0..jitter-1}, the start at 0; an arc is as
    long as the difference (0 at least: arcs the packer trims may run backwards); a final weight's string runs to
    step (depth + 1), the utterance length."""
    rng = np.random.default_rng(seed)
    n = int(lat["num_states"])
    src, dst = np.asarray(lat["src"], np.int64), np.asarray(lat["dst"], np.int64)
    level = np.full(n, -1, np.int64)
    level[int(lat["start"])] = 0
    while True:
        new = level.copy()
        ok = level[src] >= 0
        np.maximum.at(new, dst[ok], level[src[ok]] + 1)
        if np.array_equal(new, level):
            break
        level = new
    t = step * np.maximum(level, 0) + rng.integers(0, jitter, n)
    t[int(lat["start"])] = 0
    T = step * (int(level.max()) + 1)
    al = np.maximum(t[dst] - t[src], 0)
    fl = np.where(np.isfinite(np.asarray(lat["final"])), np.maximum(T - t, 0), 0)
    out = {k: v for k, v in lat.items() if k != "tid"}
    out["tid_off"] = np.concatenate([[0], np.cumsum(al)]).astype(np.int64)
    out["tids"] = np.ones(int(al.sum()), np.int32)
    out["final_acoustic"] = np.zeros(n, np.float32)
    out["final_tid_off"] = np.concatenate([[0], np.cumsum(fl)]).astype(np.int64)
    out["final_tids"] = np.ones(int(fl.sum()), np.int32)
    return out
