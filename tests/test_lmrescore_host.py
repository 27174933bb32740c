"""N-gram LM rescoring, host side: the ARPA loader and the trie tables of pykaldi2_amd.ngram against the
restatement's, the error cases, the restatement's composition against a textbook backoff scorer over enumerated paths, and
fold_finals through the archive writer and reader."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmrescore_ref as R  # noqa: E402
import mbr_ref  # noqa: E402
from pykaldi2_amd import kaldi_io, ngram, score  # noqa: E402


def _names(vocab):
    n = {w: "w%d" % w for w in range(1, vocab + 1)}
    n[vocab + 1], n[vocab + 2] = "<s>", "</s>"
    return n


@pytest.mark.parametrize("order,seed", [(1, 0), (2, 1), (3, 2), (4, 3)])
def test_arpa_round_trip_and_table_invariants(tmp_path, order, seed):
    vocab = 6
    ngrams, bos, eos = R.random_lm(vocab, order, seed)
    names = _names(vocab)
    path = str(tmp_path / "lm.arpa")
    R.write_arpa(path, ngrams, order, names)
    symbols = {names[w]: w for w in range(1, vocab + 1)}          # <s>, </s> get the ids above the table: vocab + 1, + 2
    a = ngram.NgramLM.from_arpa(path, symbols=symbols)
    b = ngram.NgramLM.from_ngrams(ngrams, bos, eos, order)
    ref = R.RefLM(ngrams, bos, eos, order)
    assert (a.bos_id, a.eos_id, a.skipped, a.order) == (bos, eos, 0, order)
    for lm in (a, b):
        assert lm.num_nodes == ref.num_nodes and lm.start == ref.start
        for k, v in ref.tables().items():
            assert lm.tables()[k].dtype == v.dtype and np.array_equal(lm.tables()[k].view(np.int32), v.view(np.int32)), k
    # invariants of the contract
    N, cb = b.num_nodes, b.child_begin
    assert cb[0] == 1 and cb[N] == N and (np.diff(cb) >= 0).all()
    has = np.diff(cb) > 0
    level = np.searchsorted(b.order_off, np.arange(N), side="right") - 1
    for i in range(N):
        w = b.word[cb[i]:cb[i + 1]]
        assert (np.diff(w) > 0).all()
        if has[i]:
            assert b.order_off[level[i] + 1] <= cb[i] and cb[i + 1] <= b.order_off[level[i] + 2]
        if i:
            assert level[b.bo_link[i]] < level[i]
            assert b.next_state[i] == 0 or has[b.next_state[i]]
            assert b.backoff[i] == 0 or has[i]                   # the generator's LMs: no backoff weight on a childless n-gram
    # arc() agrees with the restatement's on every (state, word)
    for h in [0] + [i for i in range(N) if has[i]]:
        for w in list(range(1, vocab + 1)) + [eos]:
            assert b.arc(h, w) == ref.arc(h, w)


def test_loader_errors(tmp_path):
    vocab, names = 3, _names(3)
    ngrams, bos, eos = R.random_lm(vocab, 2, 5, density=1.0)
    symbols = {names[w]: w for w in range(1, vocab + 1)}
    no_eos = {g: v for g, v in ngrams.items() if eos not in g}
    with pytest.raises(ValueError, match="end-of-sentence"):
        ngram.NgramLM.from_ngrams(no_eos, bos, eos, 2)
    p = str(tmp_path / "no_eos.arpa")
    R.write_arpa(p, no_eos, 2, names)
    with pytest.raises(ValueError, match="end-of-sentence"):
        ngram.NgramLM.from_arpa(p, symbols=symbols)
    # a trigram whose context (1, 2) is not a bigram
    broken = {g: v for g, v in ngrams.items() if g != (1, 2)}
    broken[(1, 2, 3)] = (-1.0, None)
    with pytest.raises(ValueError, match=r"\(1, 2, 3\).*\(1, 2\)"):
        ngram.NgramLM.from_ngrams(broken, bos, eos, 3)
    lm = ngram.NgramLM.from_ngrams(broken, bos, eos, 3, repair=True)
    assert lm.skipped == 1 and lm.num_nodes == len(broken)      # the empty history in place of the skipped trigram
    p = str(tmp_path / "broken.arpa")
    R.write_arpa(p, broken, 3, names)
    with pytest.raises(ValueError, match="context"):
        ngram.NgramLM.from_arpa(p, symbols=symbols)
    assert ngram.NgramLM.from_arpa(p, symbols=symbols, repair=True).skipped == 1
    # a word outside the symbol table: its n-grams are skipped and counted
    p = str(tmp_path / "full.arpa")
    R.write_arpa(p, ngrams, 2, names)
    small = {k: v for k, v in symbols.items() if k != "w3"}
    lm = ngram.NgramLM.from_arpa(p, symbols=small)
    assert lm.skipped == sum(3 in g for g in ngrams) > 0 and lm.num_nodes == 1 + sum(3 not in g for g in ngrams)
    assert lm.has_word(2) and not lm.has_word(5)
    assert (lm.bos_id, lm.eos_id) == (3, 4)                      # the ids above the (smaller) table
    # order 9
    with pytest.raises(ValueError, match="order"):
        ngram.NgramLM.from_ngrams(ngrams, bos, eos, 9)
    p = str(tmp_path / "nine.arpa")
    with open(p, "w") as f:
        f.write("\\data\\\nngram 1=3\n\n\\1-grams:\n-1 <s>\n-1 </s>\n-1 w1\n\n\\9-grams:\n-1 w1 w1 w1 w1 w1 w1 w1 w1 w1\n\\end\\\n")
    with pytest.raises(ValueError, match="order"):
        ngram.NgramLM.from_arpa(p, symbols=symbols)
    with pytest.raises(ValueError, match="unknown word"):
        ngram.NgramLM.from_arpa(str(tmp_path / "full.arpa"), symbols=symbols, unk="<unk>")


ORACLE_SHAPES = [(1, 1, 2), (2, 1, 2), (3, 2, 3), (8, 4, 5)]


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_composition_against_textbook_backoff(shape, order):
    """Every path of the composed lattice carries the textbook score of its word sequence, and the composed lattice has
    exactly the input's paths.  Tolerance: one float32 rounding per arc of a path, 2^-24 relative each, at most `depth`
    arcs: depth 2^-23 max |graph cost| leaves a factor of two for the float64 sums."""
    depth, width, vocab = shape
    for seed in range(3):
        P = score.pack_lattice(mbr_ref.random_lattice(depth, width, vocab, seed))
        ngrams, bos, eos = R.random_lm(vocab, order, 10 * seed + order)
        lm = R.RefLM(ngrams, bos, eos, order)
        scale = 0.75
        C = R.compose(P, lm, scale)
        n = C["num_states"]
        cpaths = R.paths(n, 0, C["src"], C["dst"], {n - 1})
        ipaths = R.paths(P.S, 0, P.src, P.dst, {P.S - 1})
        key = lambda words, arcs: (tuple(int(w) for w in words if w != 0), tuple(int(a) for a in arcs))
        got = sorted(key(C["word"][list(p)], C["orig_arc"][list(p)]) for p in cpaths)
        want = sorted(key(P.word_ids[P.word[list(p)]], p) for p in ipaths)
        assert got == want
        tol = P.depth * 2.0 ** -23 * max(float(np.abs(C["graph"]).max()), float(np.abs(P.graph).max()))
        for p in cpaths:
            p = list(p)
            added = float(np.sum(C["graph"][p].astype(np.float64) - P.graph[C["orig_arc"][p]].astype(np.float64)))
            words = [int(w) for w in C["word"][p] if w != 0]
            assert abs(added - scale * R.textbook_cost(ngrams, order, bos, eos, words)) <= tol, (seed, words)


def test_scale_minus_one_then_plus_one_returns_the_costs():
    """Restatement: rescoring with -1 and then +1 of the same LM gives the graph costs back to 2 float32 ulp -- the two
    roundings are half an ulp of the intermediate and half an ulp of the final cost, so the ulp is taken at the largest of
    the three magnitudes (original, intermediate, final).  With a unigram LM the composition has the input's states."""
    for order in (1, 3):
        P = score.pack_lattice(mbr_ref.random_lattice(8, 4, 5, 1))
        ngrams, bos, eos = R.random_lm(5, order, 4)
        lm = R.RefLM(ngrams, bos, eos, order)
        C1 = R.compose(P, lm, -1.0)
        if order == 1:
            assert C1["num_states"] == P.S and np.array_equal(C1["orig_arc"], np.arange(P.A))
        F = score.fold_finals(C1)
        P1 = score.pack_lattice(F)
        C2 = R.compose(P1, lm, 1.0)
        assert C2["num_states"] == C1["num_states"] and C2["src"].size == C1["src"].size
        fin = np.flatnonzero(np.isfinite(F["final"]))
        to_p = np.concatenate([F["orig_arc"], F["final_orig_arc"][fin]])[P1.orig_arc][C2["orig_arc"]]      # arc of P
        mid = np.concatenate([F["graph"], F["final"][fin]])[P1.orig_arc][C2["orig_arc"]]
        g0, g2 = P.graph[to_p], C2["graph"]
        big = np.maximum(np.abs(mid), np.maximum(np.abs(g0), np.abs(g2))).astype(np.float32)
        assert (np.abs(g2.astype(np.float64) - g0.astype(np.float64)) <= 2.0 * np.spacing(big).astype(np.float64)).all()
        assert np.array_equal(C2["acoustic"], P.acoustic[to_p])


def test_fold_finals_round_trip(tmp_path):
    lat = mbr_ref.random_lattice(8, 4, 5, 2)
    lat["tid"] = np.arange(1, lat["src"].size + 1).astype(np.int32)        # a distinct string per arc
    P = score.pack_lattice(lat)
    ngrams, bos, eos = R.random_lm(5, 2, 7)
    C = R.compose(P, R.RefLM(ngrams, bos, eos, 2), 1.0)
    # what score.rescore_lm attaches: the strings of the input's arcs along orig_arc (finals of this form have none)
    inp = np.asarray(P.orig_arc)[C["orig_arc"]]
    strs = [[int(lat["tid"][k])] if k < lat["src"].size else [] for k in inp]
    C["tid_off"] = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
    C["tids"] = np.asarray([x for s in strs for x in s], np.int32)
    C["input_arc"] = inp
    F = score.fold_finals(C)
    n = C["num_states"]
    assert F["num_states"] == n - 1 and F["src"].size + int(np.isfinite(F["final"]).sum()) == C["src"].size
    path = str(tmp_path / "lat.ark")
    with kaldi_io.CompactLatticeWriter("ark:" + path) as w:
        w["utt1"] = F
    (key, back), = list(kaldi_io.read_compact_lattice_ark(path))
    assert key == "utt1" and back["num_states"] == n - 1 and back["start"] == 0
    got = sorted((a[0], a[1], a[3], a[4][0], a[4][1], tuple(a[4][2])) for a in back["arcs"])
    want = sorted((int(F["src"][i]), int(F["dst"][i]), int(F["word"][i]), float(F["graph"][i]), float(F["acoustic"][i]),
                   tuple(int(x) for x in F["tids"][F["tid_off"][i]:F["tid_off"][i + 1]])) for i in range(F["src"].size))
    assert got == want
    for s, f in enumerate(back["finals"]):
        if np.isfinite(F["final"][s]):
            assert (f[0], f[1]) == (float(F["final"][s]), float(F["final_acoustic"][s]))
        else:
            assert f[0] == np.inf
    # the folded lattice packs to the composed lattice again: same paths, same costs
    P2 = score.pack_lattice(back)
    assert (P2.S, P2.A) == (n, C["src"].size)
    assert np.array_equal(np.sort(P2.graph), np.sort(C["graph"]))
    for i in range(F["src"].size):
        assert [int(x) for x in F["tids"][F["tid_off"][i]:F["tid_off"][i + 1]]] == \
            ([int(lat["tid"][F["input_arc"][i]])] if F["input_arc"][i] < lat["src"].size else [])
    with pytest.raises(ValueError, match="composed"):
        score.fold_finals(lat)


def test_ngram_create_validates_every_table_on_the_host():
    """pk2_ngram_create refuses malformed tables with PK2_ERR_INVALID before it touches the device (so this runs without one)."""
    import ctypes as C
    from pykaldi2_amd import _lib
    ngrams, bos, eos = R.random_lm(4, 3, 3)
    lm = ngram.NgramLM.from_ngrams(ngrams, bos, eos, 3)
    L = _lib.lib()

    def create(**kw):
        t = dict(lm.tables(), order_off=lm.order_off, N=lm.num_nodes, order=lm.order, start=lm.start, eos=lm.eos_id)
        for k, v in kw.items():
            t[k] = v(t[k].copy()) if callable(v) else v
        h = C.c_void_p()
        rc = L.pk2_ngram_create(t["N"], t["order"], _lib.ptr(t["order_off"]), _lib.ptr(t["word"]), _lib.ptr(t["cost"]),
                                _lib.ptr(t["backoff"]), _lib.ptr(t["child_begin"]), _lib.ptr(t["bo_link"]), _lib.ptr(t["next_state"]),
                                t["start"], t["eos"], None, C.byref(h))
        assert h.value is None
        return rc, (L.pk2_last_error() or b"").decode()

    def put(i, x):
        def f(a):
            a[i] = x
            return a
        return f
    has = np.diff(lm.child_begin) > 0
    parent = int(np.flatnonzero(has)[-1])                        # the last node with children: a bigram
    childless = int(np.flatnonzero(~has)[0])
    b0 = int(lm.child_begin[0])
    bad = dict(
        order=dict(order=9), nodes=dict(N=1), order_ranges=dict(order_off=put(1, 2)),
        child_not_monotone=dict(child_begin=put(parent, int(lm.child_begin[parent + 1]) + 1)),
        child_outside_next_order=dict(child_begin=put(1, b0)),   # the first unigram's range would start among the unigrams
        words_not_ascending=dict(word=put(b0 + 1, int(lm.word[b0]))),
        bo_link_not_lower=dict(bo_link=put(parent, parent)), bo_link_range=dict(bo_link=put(3, lm.num_nodes)),
        next_state_childless=dict(next_state=put(3, childless)), next_state_range=dict(next_state=put(3, -1)),
        start_childless=dict(start=childless), no_eos=dict(eos=999), cost_nan=dict(cost=put(2, np.nan)),
        backoff_inf=dict(backoff=put(2, np.inf)))
    for name, kw in bad.items():
        rc, msg = create(**kw)
        assert rc < 0 and "ngram_create" in msg and "hip" not in msg.lower(), (name, rc, msg)
    rc = L.pk2_ngram_create(lm.num_nodes, 3, None, None, None, None, None, None, None, 0, eos, None, C.byref(C.c_void_p()))
    assert rc < 0 and b"null" in L.pk2_last_error().lower()
    assert L.pk2_ngram_destroy(None) == 0
