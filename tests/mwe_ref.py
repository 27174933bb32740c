"""Host restatement of the N-best / MWE path (pykaldi2_amd/csrc/lattice_nbest.hip, reference ops/ops.py:158-241) -- test
infrastructure only.  It runs on oracle.lattice_ref.decode lattices (LatticeRef.arrays(): tokens frame by frame, kept links,
acoustic costs with the acoustic scale removed), which the existing tests show equal the device's.

  link labels      words: pk2_decode_graph_link_words restated; phones: TransitionModel.phone_label_table()
  kbest            per-token K best partial paths in np.float32 with the device's tie rule (optionally distinct labels)
  brute_force      every complete path of a tiny lattice
  edit_distance    textbook Levenshtein DP
  mwe_formula      p_k, loss, g_k and the dense gradient in float64
"""
import numpy as np

HASH0 = 1469598103934665603
M64 = (1 << 64) - 1


def hash_step(h, label):
    """nb_hash_step of lattice_nbest.hip: 64-bit hash of a label prefix."""
    if label == 0:
        return h
    z = (h ^ ((label & 0xFFFFFFFF) + 0x9E3779B97F4A7C15)) & M64
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 31
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 29
    return z


def f32_bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def link_words(graph, lat):
    """Word id of the HCLG arc behind every link: same source state, destination state and transition-id (epsilon arcs for
    transition-id 0), weight nearest the link's graph cost, the first such arc in input order; -1 when there is none."""
    src, dst, il = np.asarray(graph["src"]), np.asarray(graph["dst"]), np.asarray(graph["ilabel"])
    w, ol = np.asarray(graph["weight"], np.float32), np.asarray(graph["olabel"])
    by_src = {}
    for a in range(src.shape[0]):
        by_src.setdefault(int(src[a]), []).append(a)
    st = lat["tok_state"]
    out = np.empty(lat["link_src"].shape[0], np.int32)
    for l in range(out.shape[0]):
        s, d, t, g = int(st[lat["link_src"][l]]), int(st[lat["link_dst"][l]]), int(lat["link_tid"][l]), lat["link_graph"][l]
        best, bd = -1, np.float32(np.inf)
        for a in by_src.get(s, []):
            if int(dst[a]) != d or (int(il[a]) != t if t > 0 else int(il[a]) != 0):
                continue
            dd = np.float32(abs(np.float32(w[a]) - np.float32(g)))
            if dd < bd:
                bd, best = dd, int(ol[a])
        out[l] = best
    return out


def phone_labels(trans_model, lat):
    tab = trans_model.phone_label_table()
    return np.asarray([tab[t] if t > 0 else 0 for t in lat["link_tid"]], np.int32)


def link_costs(lat, lm, am):
    g = lat["link_graph"].astype(np.float32)
    ac = lat["link_ac"].astype(np.float32)
    return np.asarray([np.float32(np.float32(lm * float(g[l])) + np.float32(am * float(ac[l]))) for l in range(g.shape[0])],
                      np.float32)


def _topo_tokens(lat):
    """Tokens frame by frame, inside a frame in epsilon-DAG order."""
    fr, T = lat["tok_frame"], int(lat["tok_frame"].max())
    order = []
    for t in range(T + 1):
        toks = [int(i) for i in np.flatnonzero(fr == t)]
        lev = {i: 0 for i in toks}
        eps = [l for l in range(lat["link_src"].shape[0]) if lat["link_tid"][l] == 0 and fr[lat["link_src"][l]] == t]
        for _ in range(len(toks) + 1):
            changed = False
            for l in eps:
                s, d = int(lat["link_src"][l]), int(lat["link_dst"][l])
                if lev[s] + 1 > lev[d]:
                    lev[d] = lev[s] + 1
                    changed = True
            if not changed:
                break
        order.extend(sorted(toks, key=lambda i: (lev[i], i)))
    return order


def kbest(lat, labels, K, lm=1.0, am=1.0, distinct=False):
    """Per-token K best partial paths and the final top K, with the device's tie rule.  Returns a list of
    (labels, tids, cost) in ascending cost; in reference mode paths that repeat an earlier path's labels are dropped."""
    A = lat
    fr, st = A["tok_frame"], A["tok_state"]
    T = int(fr.max())
    start = int(A.get("start_tok", 0))
    c = link_costs(A, lm, am)
    inc = {}
    for l in range(A["link_src"].shape[0]):
        inc.setdefault(int(A["link_dst"][l]), []).append(l)
    lists = {start: [(np.float32(0.0), -1, 0, HASH0)]}      # (cost, link, source rank, hash)

    def select(cands):
        cands.sort(key=lambda x: x[0])
        out, seen = [], set()
        for _, e in cands:
            if distinct and e[3] in seen:
                continue
            seen.add(e[3])
            out.append(e)
            if len(out) == K:
                break
        return out

    for d in _topo_tokens(A):
        if d == start:
            continue
        cands = []
        for l in inc.get(d, []):
            s = int(A["link_src"][l])
            fbit = 1 if fr[s] == fr[d] else 0
            for r, e in enumerate(lists.get(s, [])):
                cost = np.float32(e[0] + c[l])
                key = (float(cost), fbit, int(st[s]), int(A["link_tid"][l]), f32_bits(A["link_graph"][l]), r)
                cands.append((key, (cost, l, r, hash_step(e[3], int(labels[l])))))
        lists[d] = select(cands)
    cands = []
    for i in np.flatnonzero(fr == T):
        f = A["tok_final"][i]
        if not np.isfinite(f):
            continue
        add = np.float32(lm * float(f))
        for r, e in enumerate(lists.get(int(i), [])):
            cost = np.float32(e[0] + add)
            cands.append(((float(cost), int(st[i]), r), (cost, int(i), r, e[3])))
    final = select(cands)
    paths = []
    for cost, tok, r, _ in final:
        labs, tids = [], []
        while True:
            e = lists[tok][r]
            if e[1] < 0:
                break
            l = e[1]
            if A["link_tid"][l] > 0:
                tids.append(int(A["link_tid"][l]))
            if labels[l] != 0:
                labs.append(int(labels[l]))
            tok, r = int(A["link_src"][l]), e[2]
        paths.append((labs[::-1], np.asarray(tids[::-1], np.int32), float(cost)))
    if distinct:
        return paths
    out, seen = [], []
    for p in paths:
        if p[0] not in seen:
            seen.append(p[0])
            out.append(p)
    return out


def brute_force(lat, labels, lm=1.0, am=1.0):
    """Every complete path of a (tiny) lattice: (labels, tids, cost) sorted by cost."""
    A = lat
    fr = A["tok_frame"]
    T = int(fr.max())
    c = link_costs(A, lm, am)
    out_links = {}
    for l in range(A["link_src"].shape[0]):
        out_links.setdefault(int(A["link_src"][l]), []).append(l)
    res = []

    def walk(tok, cost, labs, tids):
        if fr[tok] == T and np.isfinite(A["tok_final"][tok]):
            res.append((list(labs), np.asarray(tids, np.int32), float(np.float32(cost + np.float32(lm * float(A["tok_final"][tok]))))))
        for l in out_links.get(tok, []):
            lb, t = int(labels[l]), int(A["link_tid"][l])
            walk(int(A["link_dst"][l]), np.float32(cost + c[l]), labs + ([lb] if lb else []), tids + ([t] if t else []))
            if len(res) > 200000:
                raise RuntimeError("lattice too large for brute force")

    walk(int(A.get("start_tok", 0)), np.float32(0.0), [], [])
    res.sort(key=lambda p: p[2])
    return res


def edit_distance(a, b):
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[-1]


def mwe_formula(hyps, supervision, tid2pdf, T, P, equal_weight):
    """hyps = [(labels, tids, cost)] -> (loss, grad f64 [T, P]) by the reference's formula in float64."""
    M = len(hyps)
    e = np.asarray([edit_distance(h[0], supervision) for h in hyps], np.float64)
    w = np.asarray([h[2] for h in hyps], np.float64)
    if equal_weight:
        p = np.full(M, 1.0 / M)
    else:
        x = np.exp(-(w - w.min()))
        p = x / x.sum()
    loss = float((e * p).sum())
    g = (e - loss) * p
    grad = np.zeros((T, P), np.float64)
    for k, h in enumerate(hyps):
        for t, tid in enumerate(h[1][:T]):
            grad[t, tid2pdf[tid]] += g[k]
    return loss, grad
