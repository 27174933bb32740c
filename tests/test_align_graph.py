"""Training graphs of the forced aligner (csrc/align_graph.hip), checked on the host against an independent construction:
every phone string the lexicon allows for the transcript is enumerated by brute force, expanded into its context-dependent
HMM chain, and aligned by a float64 Viterbi; the best of them must be what a float64 Viterbi over the compiled graph finds.
Also: <LogProbs> of text and binary transition models, and the error cases.  No GPU needed.

The helpers here (model builders, Viterbi references, the f32 emulation of the device kernel) are shared with
tests/test_gpu_align.py and tests/test_gpu_cli_se2.py."""
import re
import struct

import numpy as np
import pytest

from pykaldi2_amd import chain, lattice, synth
from pykaldi2_amd.tree import ContextDependency

from recipe import write_fst_vector

INF = float("inf")


# ---------------------------------------------------------------- writers
def write_trans_model_text(path, tm):
    by_entry = {}
    for ph, e in sorted(tm.phone2entry.items()):
        by_entry.setdefault(e, []).append(ph)
    lines = ["<TransitionModel>", "<Topology>"]
    for e, phones in sorted(by_entry.items()):
        lines += ["<TopologyEntry>", "<ForPhones>", " ".join(map(str, phones)), "</ForPhones>"]
        for hs, (f, l, dsts) in enumerate(tm.entries[e]):
            if not dsts:
                lines.append("<State> %d </State>" % hs)
                continue
            tr = " ".join("<Transition> %d %.4f" % (d, 1.0 / len(dsts)) for d in dsts)
            lines.append("<State> %d <ForwardPdfClass> %d <SelfLoopPdfClass> %d %s </State>" % (hs, f, l, tr))
        lines.append("</TopologyEntry>")
    lines += ["</Topology>", "<Tuples> %d" % len(tm.tuples)]
    lines += ["%d %d %d %d" % tuple(int(v) for v in t) for t in tm.tuples]
    lines += ["</Tuples>", "<LogProbs>", " [ " + " ".join(repr(float(v)) for v in tm.log_probs) + " ]", "</LogProbs>",
              "</TransitionModel>"]
    open(path, "w").write("\n".join(lines) + "\n")


def write_trans_model_binary(path, tm):
    """Kaldi's binary TransitionModel [upstream knowledge: TransitionModel::Write, HmmTopology::Write in the non-HMM form,
    Vector<float>::Write]."""
    out = bytearray(b"\0B")
    tok = lambda t: out.extend((t + " ").encode())                      # noqa: E731
    i32 = lambda v: out.extend(struct.pack("<bi", 4, int(v)))            # noqa: E731
    f32 = lambda v: out.extend(struct.pack("<bf", 4, float(v)))          # noqa: E731

    def ivec(v):
        out.extend(struct.pack("<bi", 4, len(v)) + struct.pack("<%di" % len(v), *[int(x) for x in v]))
    tok("<TransitionModel>"); tok("<Topology>")
    phones = sorted(tm.phone2entry)
    ivec(phones)
    p2i = [-1] * (max(phones) + 1)
    for p in phones:
        p2i[p] = tm.phone2entry[p]
    ivec(p2i)
    i32(-1); i32(len(tm.entries))
    for states in tm.entries:
        i32(len(states))
        for f, l, dsts in states:
            i32(f); i32(l); i32(len(dsts))
            for d in dsts:
                i32(d); f32(1.0 / len(dsts))
    tok("</Topology>"); tok("<Tuples>"); i32(len(tm.tuples))
    for t in tm.tuples:
        for v in t:
            i32(v)
    tok("</Tuples>"); tok("<LogProbs>"); tok("FV"); i32(len(tm.log_probs))
    out.extend(np.asarray(tm.log_probs, "<f4").tobytes())
    tok("</LogProbs>"); tok("</TransitionModel>")
    open(path, "wb").write(bytes(out))


def write_lexicon(path, lex):
    write_fst_vector(path, lex["num_states"], lex["start"], lex["src"], lex["dst"], lex["ilabel"], lex["olabel"],
                     lex["weight"], lex["final"])


# ---------------------------------------------------------------- models
TOPOS = [synth.CHAIN_TOPO, synth.BAKIS_TOPO, synth.SKIP_TOPO]


def random_log_probs(tm, rng):
    lp = np.zeros(tm.num_transition_ids() + 1)
    for ts in range(1, int(tm.tid2tstate.max()) + 1):
        ids = np.flatnonzero(tm.tid2tstate == ts)
        p = rng.dirichlet(np.full(len(ids), 2.0))
        lp[ids] = np.log(np.maximum(p, 1e-3) / np.maximum(p, 1e-3).sum())
    return lp


def make_model(num_phones, N, P, seed=0, mixed=True, num_pdfs=60):
    """A tree with window (N, P) -- tables over the window positions, then the pdf-class -- with random pdfs, the
    tuples it can produce, and random non-uniform log-probabilities.  Phone 1 is silence (Bakis)."""
    rng = np.random.default_rng(seed)
    phone2entry = {p: ((1 if p % 3 == 0 else 2 if p % 5 == 0 else 0) if mixed else 1) for p in range(1, num_phones + 1)}
    phone2entry[1] = 1
    order = [P] + [k for k in range(N) if k != P]
    leaf = {}

    def build(level, window):
        if level == len(order):
            p = window[P]
            classes = sorted({c for f, l, _ in TOPOS[phone2entry[p]][:-1] for c in (f, l)})
            kids = [None] * (max(classes) + 1)
            for c in classes:
                pdf = int(rng.integers(0, num_pdfs))
                kids[c] = ("CE", pdf)
                leaf[(tuple(window[k] for k in range(N)), c)] = pdf
            return ("TE", -1, kids)
        key = order[level]
        vals = range(1, num_phones + 1) if key == P else range(0, num_phones + 1)
        kids = [None] * (num_phones + 1)
        for v in vals:
            w = dict(window)
            w[key] = v
            kids[v] = build(level + 1, w)
        return ("TE", key, kids)

    tree = ContextDependency.from_nested(N, P, build(0, {}))
    tuples = set()
    windows = {w for (w, _) in leaf}
    for w in windows:
        p = w[P]
        for hs, (f, l, _) in enumerate(TOPOS[phone2entry[p]][:-1]):
            tuples.add((p, hs, leaf[(w, f)], leaf[(w, l)]))
    tm = lattice.TransitionModel.from_topology(phone2entry, TOPOS, sorted(tuples))
    tm.log_probs = random_log_probs(tm, rng)
    return tree, tm


def kaldi_like_lexicon(prons, sil_phone=1, sil_prob=0.3, disambig=None):
    """L.fst shaped like Kaldi's utils/make_lexicon_fst.py with optional silence: start -> loop state with or without
    silence, every pronunciation (word on the first arc, its cost there) back to the loop state, optionally through the
    silence state.  prons: [(word, [phones], cost, disambig symbol or None)]."""
    src, dst, il, ol, w = [], [], [], [], []
    add = lambda a, b, i, o, c: (src.append(a), dst.append(b), il.append(i), ol.append(o), w.append(c))   # noqa: E731
    ns_cost, s_cost = -np.log(1 - sil_prob), -np.log(sil_prob)
    start, loop, sil = 0, 1, 2
    n = 3
    add(start, loop, 0, 0, ns_cost)
    add(start, sil, 0, 0, s_cost)
    add(sil, loop, sil_phone, 0, 0.0)
    for word, phones, cost, dis in prons:
        seq = list(phones) + ([dis] if dis else [])
        cur = loop
        for j, p in enumerate(seq[:-1]):
            add(cur, n, p, word if j == 0 else 0, cost if j == 0 else 0.0)
            cur, n = n, n + 1
        last = seq[-1]
        o = word if len(seq) == 1 else 0
        c = cost if len(seq) == 1 else 0.0
        add(cur, loop, last, o, c + ns_cost)
        add(cur, sil, last, o, c + s_cost)
    final = np.full(n, np.inf, np.float32)
    final[loop] = 0.0
    return dict(num_states=n, start=start, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                ilabel=np.asarray(il, np.int32), olabel=np.asarray(ol, np.int32), weight=np.asarray(w, np.float32), final=final)


# ---------------------------------------------------------------- brute force
def lexicon_paths(lex, words, disambig=(), max_depth=64):
    """Every path of L that outputs exactly `words`: (phones, per-phone cost = epsilon costs since the last phone + its arc,
    final cost = trailing epsilon costs + final weight), costs in float64 summed along the path."""
    dis = set(disambig)
    arcs = {}
    for k in range(len(lex["src"])):
        arcs.setdefault(int(lex["src"][k]), []).append(k)
    out = []

    def walk(s, j, pending, phones, costs, depth):
        if depth > max_depth:
            raise RuntimeError("lexicon path too deep")
        if j == len(words) and np.isfinite(lex["final"][s]):
            out.append((tuple(phones), tuple(costs), pending + float(lex["final"][s])))
        for k in arcs.get(s, []):
            o, i = int(lex["olabel"][k]), int(lex["ilabel"][k])
            if o != 0 and (j >= len(words) or o != words[j]):
                continue
            nj = j + (o != 0)
            c = pending + float(lex["weight"][k])
            if i == 0 or i in dis:
                walk(int(lex["dst"][k]), nj, c, phones, costs, depth + 1)
            else:
                walk(int(lex["dst"][k]), nj, 0.0, phones + [i], costs + [c], depth + 1)
    walk(int(lex["start"]), 0, 0.0, [], [], 0)
    return out


def hmm_chain(tree, tm, phones, costs, final, tscale, lscale):
    """The aligner's graph of ONE phone string, built from the definition (Kaldi's H with reordered self-loops): states
    (i, s, q) = phone i, HMM state s left by transition q; arcs (dst, src, tid, pdf, f32 weight), src -1 = start."""
    first = {}
    tid = 1
    for t in tm.tuples.tolist():
        first[tuple(t)] = tid
        tid += len(tm.entries[tm.phone2entry[t[0]]][t[1]][2])
    N, P = tree.N, tree.P
    m = len(phones)
    states, index = [], {}
    info = {}
    for i, p in enumerate(phones):
        win = [(phones[i - P + k] if 0 <= i - P + k < m else 0) for k in range(N)]
        topo = tm.entries[tm.phone2entry[p]]
        ns = len(topo) - 1
        for s in range(ns):
            f, l, dsts = topo[s]
            fp, lp = tree.compute(win, f), tree.compute(win, l)
            t0 = first[(p, s, fp, lp)]
            loop = [q for q, d in enumerate(dsts) if d == s]
            tl = t0 + loop[0] if loop else 0
            one_minus = np.log1p(-np.exp(tm.log_probs[tl])) if loop else 0.0
            lw = lscale * -tm.log_probs[tl] if loop else 0.0
            for q, d in enumerate(dsts):
                if d == s:
                    continue
                fw = tscale * (-tm.log_probs[t0 + q] + one_minus) + lscale * -one_minus
                index[(i, s, q)] = len(states)
                states.append((i, s, q, d, ns))
                info[(i, s, q)] = (t0 + q, fp, fw, tl, lp, lw)
    arcs = []
    for x, (i, s, q, d, ns) in enumerate(states):
        tf, fp, fw, tl, lp, lw = info[(i, s, q)]
        if tl:
            arcs.append((x, x, tl, lp, np.float32(lw)))
        if s == 0:
            if i == 0:
                arcs.append((x, -1, tf, fp, np.float32(costs[0] + fw)))
            else:
                for y, (i2, s2, q2, d2, ns2) in enumerate(states):
                    if i2 == i - 1 and d2 == ns2:
                        arcs.append((x, y, tf, fp, np.float32(costs[i] + fw)))
        for y, (i2, s2, q2, d2, ns2) in enumerate(states):
            if i2 == i and d2 == s:
                arcs.append((x, y, tf, fp, np.float32(fw)))
    fin = np.full(len(states), np.inf)
    for x, (i, s, q, d, ns) in enumerate(states):
        if i == m - 1 and d == ns:
            fin[x] = np.float32(final)
    return len(states), arcs, fin


def viterbi64(S, arcs, fin, ll, ascale):
    """float64 Viterbi, no beam: arcs (dst, src, tid, pdf, weight).  -> (best cost, transition-ids) or (inf, None)."""
    T = ll.shape[0]
    dst = np.asarray([a[0] for a in arcs]); src = np.asarray([a[1] for a in arcs])
    tid = np.asarray([a[2] for a in arcs]); pdf = np.asarray([a[3] for a in arcs])
    w = np.asarray([float(a[4]) for a in arcs])
    cost = np.full(S, np.inf)
    bps = []
    for t in range(T):
        prev = np.where(src < 0, 0.0 if t == 0 else np.inf, cost[np.maximum(src, 0)])
        cand = prev + w - ascale * ll[t, pdf].astype(np.float64)
        new = np.full(S, np.inf)
        np.minimum.at(new, dst, cand)
        bp = np.full(S, -1)
        hit = np.flatnonzero((cand == new[dst]) & np.isfinite(cand))[::-1]
        bp[dst[hit]] = hit                    # the last write wins: the lowest arc of a tie
        cost = new
        bps.append(bp)
    tot = cost + fin
    s = int(np.argmin(tot))
    if not np.isfinite(tot[s]):
        return np.inf, None
    path = []
    for t in range(T - 1, -1, -1):
        k = bps[t][s]
        path.append(int(tid[k]))
        s = int(src[k])
    return float(tot.min()), path[::-1]


def exported_arcs(g):
    return [(int(d), int(s), int(t), int(p), np.float32(w)) for d, s, t, p, w in zip(g["dst"], g["src"], g["tid"], g["pdf"], g["weight"])]


def brute_force(tree, tm, lex, words, ll, ascale, tscale, lscale, disambig=()):
    best, best_tids = np.inf, None
    for phones, costs, final in lexicon_paths(lex, words, disambig):
        S, arcs, fin = hmm_chain(tree, tm, phones, costs, final, tscale, lscale)
        c, tids = viterbi64(S, arcs, fin, ll, ascale)
        if c < best:
            best, best_tids = c, tids
    return best, best_tids


# ---------------------------------------------------------------- f32 emulation of csrc/align_viterbi.hip
def emulate_viterbi(g, ll, ascale, beam, trace=None):
    """Bit-exact numpy model of the device kernel on an exported graph: -> (status, tids, total, graph, acoustic).
    trace: a dict that receives what the run met -- arc_ties (frame/state pairs where a later in-arc equalled the finite
    best so far, which strict < leaves to the earlier arc), pruned (source costs the beam turned into +inf), final_ties
    (final states with the least finite total) and, when a path was found, margin (the largest amount by which a state
    of the chosen path exceeded its frame's best cost: a smaller beam prunes that path)."""
    f = np.float32
    arc_ties = pruned = 0
    S = g["final"].shape[0]
    T = ll.shape[0]
    off, src, w, pdf, tid = g["in_off"], g["src"], g["weight"].astype(f), g["pdf"], g["tid"]
    nscale = f(-ascale)
    deg = np.diff(off)
    K = int(deg.max()) if S else 0
    cost = np.full(S, np.inf, f)
    thr = f(np.inf)
    bps = np.zeros((T, S), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            ac = (nscale * ll[t].astype(f)).astype(f)
            best = np.full(S, np.inf, f)
            arg = np.zeros(S, np.int64)
            for k in range(K):
                has = deg > k
                a = off[:-1][has] + k
                sa = src[a]
                v = np.where(sa < 0, f(0.0) if t == 0 else f(np.inf), cost[np.maximum(sa, 0)]).astype(f)
                if trace is not None:
                    pruned += int(((v > thr) & (v < np.inf)).sum())
                v = np.where(v > thr, f(np.inf), v).astype(f)
                cand = ((v + w[a]).astype(f) + ac[pdf[a]]).astype(f)
                idx = np.flatnonzero(has)
                if trace is not None:
                    arc_ties += int(((cand == best[idx]) & (cand < np.inf)).sum())
                better = cand < best[idx]
                best[idx[better]] = cand[better]
                arg[idx[better]] = a[better]
            cost = best
            bps[t] = arg
            if trace is not None:
                trace.setdefault("costs", []).append(cost)
            thr = f(np.fmin.reduce(cost) + f(beam))
        v = np.where(cost > thr, f(np.inf), cost).astype(f)
        tot = (v + g["final"].astype(f)).astype(f)
    s = int(np.argmin(tot))
    if trace is not None:
        costs = trace.pop("costs")
        trace.update(arc_ties=arc_ties, pruned=pruned, final_ties=int((tot == tot[s]).sum()) if tot[s] < np.inf else 0)
    if not tot[s] < np.inf:
        return 1, None, np.inf, np.inf, np.inf
    path = np.zeros(T, np.int64)
    excess = np.zeros(T)
    x = s
    for t in range(T - 1, -1, -1):
        path[t] = bps[t][x]
        if trace is not None:
            excess[t] = float(costs[t][x]) - float(np.fmin.reduce(costs[t]))
        x = int(src[path[t]])
    if trace is not None:
        trace.update(excess=excess, margin=float(excess.max()))
    gs, acs = f(0.0), f(0.0)
    for t in range(T):
        gs = f(gs + w[path[t]])
        acs = f(acs + f(nscale * f(ll[t, pdf[path[t]]])))
    return 0, tid[path].astype(np.int32), tot[s], f(gs + f(g["final"][s])), acs


# ---------------------------------------------------------------- tests
def test_log_probs_round_trip(tmp_path):
    tree, tm = make_model(7, 2, 1, seed=3)
    assert np.ptp(tm.log_probs[1:]) > 0.5           # non-uniform
    write_trans_model_text(str(tmp_path / "m.txt"), tm)
    write_trans_model_binary(str(tmp_path / "m.bin"), tm)
    for name in ("m.txt", "m.bin"):
        back = lattice.TransitionModel.read(str(tmp_path / name))
        assert np.array_equal(back.tid2pdf, tm.tid2pdf) and np.array_equal(back.tid_flags, tm.tid_flags)
        assert back.log_probs.dtype == np.float64 and back.log_probs.shape == tm.log_probs.shape
        want = tm.log_probs.astype(np.float32) if name == "m.bin" else tm.log_probs      # FV holds f32; text keeps repr()
        assert np.array_equal(back.log_probs, want.astype(np.float64))
    assert lattice.TransitionModel.from_arrays(synth.transition_model_arrays(30)).log_probs is None
    assert lattice.TransitionModel.from_topology(tm.phone2entry, tm.entries, tm.tuples.tolist()).log_probs is None


PRONS = [(1, [1], 0.0, None),                   # silence word
         (2, [2, 3, 4], 0.2, 9),                # homophone of word 3's first pronunciation: disambig #1 = 9
         (3, [2, 3, 4], 0.1, 10),
         (3, [5, 3], 0.9, None),
         (4, [6], 0.3, None),                   # one-phone word
         (4, [7, 6], 0.05, None),
         (5, [4, 5, 2, 6], 0.0, None)]


@pytest.mark.parametrize("N,P", [(1, 0), (2, 1), (2, 0), (3, 1)])
def test_graph_matches_brute_force(tmp_path, N, P):
    tree, tm = make_model(7, N, P, seed=N * 10 + P)
    tree.write(str(tmp_path / "tree"))
    tree = ContextDependency.read(str(tmp_path / "tree"))
    lex = kaldi_like_lexicon(PRONS)
    write_lexicon(str(tmp_path / "L.fst"), lex)
    rng = np.random.default_rng(N + P)
    tscale, lscale, ascale = 1.0, 0.1, 0.1
    model = chain.AlignModel(tree, tm, tscale, lscale)
    lexicon = chain.Lexicon(str(tmp_path / "L.fst"), [9, 10])
    for words in ([4], [2, 4], [3, 5, 4], [4, 4, 1, 3]):
        T = 10 * len(words) + 12
        g = chain.AlignmentGraphs(model, lexicon, [words], [T])
        assert g.status == [0], g.errors
        ex = g.export(0)
        for trial in range(2):
            ll = rng.standard_normal((T, 60)).astype(np.float32) * 3
            want, want_tids = brute_force(tree, tm, lex, words, ll, ascale, tscale, lscale, disambig=[9, 10])
            got, got_tids = viterbi64(ex["final"].shape[0], exported_arcs(ex), ex["final"].astype(np.float64), ll, ascale)
            assert np.isfinite(want)
            assert abs(got - want) <= 1e-9 * abs(want), (words, got, want)
            assert got_tids == want_tids
            ok, phones = chain.split_to_phones(tm, got_tids)
            assert ok


def test_mixed_topologies_chain_model():
    tree, tm = synth.chain_model(120, seed=4, mixed_topologies=True)
    rng = np.random.default_rng(5)
    tm.log_probs = random_log_probs(tm, rng)
    nph = len(tm.phone2entry)
    prons = [(w, [int(p) for p in rng.integers(1, nph + 1, size=int(rng.integers(1, 4)))], float(rng.uniform(0, 1)), None)
             for w in range(1, 7)]
    prons.append((3, [2, 5], 0.4, None))
    lex = kaldi_like_lexicon(prons, sil_phone=3, sil_prob=0.4)
    model = chain.AlignModel(tree, tm, 1.0, 0.1)
    lexicon = chain.Lexicon(lex)
    for words in ([1, 3], [6, 2, 3]):
        T = 30
        g = chain.AlignmentGraphs(model, lexicon, [words], [T])
        assert g.status == [0], g.errors
        ex = g.export(0)
        ll = rng.standard_normal((T, 120)).astype(np.float32) * 3
        want, want_tids = brute_force(tree, tm, lex, words, ll, 0.1, 1.0, 0.1)
        got, got_tids = viterbi64(ex["final"].shape[0], exported_arcs(ex), ex["final"].astype(np.float64), ll, 0.1)
        assert abs(got - want) <= 1e-9 * abs(want) and got_tids == want_tids


def test_errors(tmp_path):
    tree, tm = make_model(7, 2, 1, seed=1)
    lexicon = chain.Lexicon(kaldi_like_lexicon(PRONS))
    model = chain.AlignModel(tree, tm)
    g = chain.AlignmentGraphs(model, lexicon, [[2, 77], [5, 5, 5, 5], [4]], [40, 12, 40])
    assert g.status == [chain.ALIGN_ERROR, chain.ALIGN_NO_PATH, chain.ALIGN_OK]
    assert "77" in g.errors[0] and "not an output label" in g.errors[0]
    assert "no path of 12 frames" in g.errors[1]
    # a window of 4 phones is refused
    t4 = ContextDependency.from_nested(4, 1, ("CE", 0))
    with pytest.raises(RuntimeError, match="context windows"):
        chain.AlignModel(t4, tm)
    # the aligner of the chain recipe (empty L.fst) builds; it fails only when asked to align
    open(tmp_path / "final.mdl", "w").close()
    write_trans_model_text(str(tmp_path / "final.mdl"), tm)
    tree.write(str(tmp_path / "tree"))
    open(tmp_path / "L.fst", "wb").close()
    open(tmp_path / "disambig.int", "w").close()
    a = chain.MappedAligner.from_files(str(tmp_path / "final.mdl"), str(tmp_path / "tree"), str(tmp_path / "L.fst"), None,
                                       str(tmp_path / "disambig.int"), None, beam=10, transition_scale=1.0,
                                       self_loop_scale=0.1, acoustic_scale=0.1)
    assert a.transition_model.log_probs is not None
    with pytest.raises(RuntimeError, match="L.fst"):
        a.align(np.zeros((20, 60), np.float32), [4])
    with pytest.raises(RuntimeError, match="needs a lexicon"):
        chain.MappedAligner(tm).align(np.zeros((20, 60), np.float32), [4])


def test_synthetic_lexicon_matches_decoding_graph():
    """synth.lexicon_arcs replays decoding_graph_arcs: the phones of every word agree."""
    P = 30
    hclg = synth.decoding_graph_arcs(25, P, seed=3, max_phones=3)
    lex = synth.lexicon_arcs(25, P, seed=3, max_phones=3)
    tm = synth.transition_model_arrays(P)
    for word in range(1, 26):
        k = int(np.flatnonzero(hclg["olabel"] == word)[0])
        s, phones = int(hclg["dst"][k]), []
        while True:
            fwd = [a for a in np.flatnonzero(hclg["src"] == s) if hclg["dst"][a] != s]
            a = fwd[0]
            if hclg["ilabel"][a] == 0:
                break
            if (hclg["ilabel"][a] - 1) % 6 == 5:          # forward id of the last HMM state: one phone done
                phones.append(int(tm["tid2phone"][hclg["ilabel"][a]]))
            s = int(hclg["dst"][a])
        paths = lexicon_paths(lex, [word])
        assert [list(p[0]) for p in paths] == [phones]
    tree, am = synth.alignment_model(P)
    g = chain.AlignmentGraphs(chain.AlignModel(tree, am), chain.Lexicon(lex), [[2, 3], [4]], [60, 30])
    assert g.status == [0, 0]


def test_state_limit():
    """kAlignMaxStates = 32 * 512 (align_internal.h): a transcript just under it compiles, a longer one is refused with
    status 3 and a message that names both numbers, and the other utterances of the call are what they are alone."""
    import graph_cases as GC
    model, lexicon = GC.triphone()
    under, over = GC.ladder_words(800), GC.ladder_words(810)
    texts, frames = [[2, 4], over, under, [4]], [40, 4000, 4000, 30]
    g = chain.AlignmentGraphs(model, lexicon, texts, frames)
    assert g.status == [chain.ALIGN_OK, chain.ALIGN_ERROR, chain.ALIGN_OK, chain.ALIGN_OK], g.errors
    S = g.num_states[2]
    assert 16000 < S <= GC.MAX_STATES == 16384, S
    assert GC.states_per_thread(S) == 32 and not g.uses_lds()
    assert g.num_states[1] == 0 and g.num_arcs[1] == 0
    m = re.search(r"has (\d+) states, more than (\d+)", g.errors[1])
    assert m and int(m.group(1)) > 16384 and int(m.group(2)) == 16384, g.errors[1]
    assert g.errors[0] == g.errors[2] == g.errors[3] == ""
    for n in (0, 2, 3):
        alone = chain.AlignmentGraphs(model, lexicon, [texts[n]], [frames[n]])
        assert alone.status == [chain.ALIGN_OK]
        a, b = alone.export(0), g.export(n)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    # the refused transcript alone: the same status, nothing compiled, nothing to launch on
    alone = chain.AlignmentGraphs(model, lexicon, [over], [4000])
    assert alone.status == [chain.ALIGN_ERROR] and alone.num_states == [0] and alone.errors[0] == g.errors[1]
