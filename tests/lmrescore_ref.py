"""Pure-Python restatement of n-gram LM rescoring (pykaldi2_amd/ngram.py, csrc/lattice_lmrescore.hip): the
trie tables in the contract's numbering, arc(h, w) with the float64 sums in the contract's order, the composition of a
packed lattice with the LM in the contract's state and arc order -- and, independent of all of it, a textbook backoff
scorer over the full history, a seeded LM generator and an ARPA writer."""
import math

import numpy as np

LN10 = math.log(10.0)


class RefLM:
    """The tables of the contract, built the slow way from {tuple of word ids: (log10 p, log10 backoff or None)}."""

    def __init__(self, ngrams, bos_id, eos_id, order):
        self.ngrams, self.bos_id, self.eos_id, self.order = dict(ngrams), bos_id, eos_id, order
        grams = [()]
        node_of = {(): 0}
        for k in range(1, order + 1):
            level = sorted((g for g in ngrams if len(g) == k), key=lambda g: (node_of[g[:-1]], g[-1]))
            for g in level:
                node_of[g] = len(grams)
                grams.append(g)
        N = len(grams)
        self.grams, self.node_of, self.num_nodes = grams, node_of, N
        kids = [[] for _ in range(N)]
        for i in range(1, N):
            kids[node_of[grams[i][:-1]]].append(i)
        self.word = np.zeros(N, np.int32)
        self.cost, self.backoff = np.zeros(N, np.float32), np.zeros(N, np.float32)
        self.bo_link, self.next_state = np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.child_begin = np.zeros(N + 1, np.int32)
        nxt = N
        self.child_begin[N] = N
        for i in range(N - 1, -1, -1):
            if kids[i]:
                assert kids[i] == list(range(kids[i][0], kids[i][-1] + 1))
                nxt = kids[i][0]
            self.child_begin[i] = nxt
        for i in range(1, N):
            g = grams[i]
            lp, bo = ngrams[g]
            self.word[i] = g[-1]
            self.cost[i] = np.float32(-LN10 * lp)
            self.backoff[i] = np.float32(-LN10 * bo) if bo is not None else np.float32(0)
            sufs = [g[j:] for j in range(1, len(g))]
            self.bo_link[i] = next((node_of[s] for s in sufs if s in node_of), 0)
            cands = ([g] if len(g) < order else []) + sufs
            self.next_state[i] = next((node_of[s] for s in cands if s in node_of and kids[node_of[s]]), 0)
        self.start = int(self.next_state[node_of[(bos_id,)]])

    def tables(self):
        return dict(word=self.word, cost=self.cost, backoff=self.backoff, child_begin=self.child_begin,
                    bo_link=self.bo_link, next_state=self.next_state)

    def child(self, node, w):
        lo, hi = int(self.child_begin[node]), int(self.child_begin[node + 1])
        while lo < hi:
            mid = (lo + hi) // 2
            if self.word[mid] < w:
                lo = mid + 1
            else:
                hi = mid
        return lo if lo < self.child_begin[node + 1] and self.word[lo] == w else -1

    def arc(self, h, w):
        acc, node = 0.0, int(h)
        while True:
            c = self.child(node, w)
            if c >= 0:
                return acc + float(self.cost[c]), int(self.next_state[c])
            assert node != 0, "word %d has no unigram" % w
            acc += float(self.backoff[node])
            node = int(self.bo_link[node])

    def final(self, h):
        return self.arc(h, self.eos_id)[0]

    def backoffs_taken(self, h, w):
        """How many times arc(h, w) backs off."""
        n, node = 0, int(h)
        while self.child(node, w) < 0:
            node, n = int(self.bo_link[node]), n + 1
        return n


def textbook_cost(ngrams, order, bos_id, eos_id, words):
    """-ln p(words </s> | <s>) by the textbook recursion over the full history (the last order - 1 words):
    p(w | h) = p(h w) if the n-gram exists, else bo(h) p(w | h without its first word), bo(h) = 1 where absent.  The
    table values are rounded to float32 as the tries hold them; the sum is float64."""
    def term(hist, w):
        g = hist + (w,)
        if g in ngrams:
            return float(np.float32(-LN10 * ngrams[g][0]))
        assert hist, "word %d has no unigram" % w
        bo = ngrams[hist][1] if hist in ngrams else None
        return (float(np.float32(-LN10 * bo)) if bo is not None else 0.0) + term(hist[1:], w)
    total, hist = 0.0, (bos_id,)
    for w in list(words) + [eos_id]:
        hist = hist[max(0, len(hist) - (order - 1)):] if order > 1 else ()
        total += term(hist, w)
        hist = hist + (w,)
    return total


def random_lm(vocab, order, seed, density=0.5):
    """Seeded n-grams over the words 1..vocab, <s> = vocab + 1, </s> = vocab + 2: every unigram; higher orders prefix- and
    suffix-closed; <s> only first, </s> only last; a backoff weight exactly on the n-grams that have children."""
    rng = np.random.default_rng(seed)
    bos, eos = vocab + 1, vocab + 2
    levels = [set(), {(w,) for w in list(range(1, vocab + 1)) + [bos, eos]}]
    for k in range(2, order + 1):
        cur = set()
        for g in sorted(levels[k - 1]):
            if eos in g or bos in g[1:]:
                continue
            for w in list(range(1, vocab + 1)) + [eos]:
                if g[1:] + (w,) in levels[k - 1] and rng.random() < density:
                    cur.add(g + (w,))
        levels.append(cur)
    allg = set().union(*levels)
    parents = {g[:-1] for g in allg if len(g) > 1}
    ngrams = {}
    for g in sorted(allg, key=lambda g: (len(g), g)):
        lp = -0.1 - 2.9 * rng.random()
        bo = -0.05 - 1.5 * rng.random()
        ngrams[g] = (float(lp), float(bo) if g in parents else None)
    return ngrams, bos, eos


def write_arpa(path, ngrams, order, names):
    """names: {word id: string}"""
    with open(path, "w") as f:
        f.write("\n\\data\\\n")
        for k in range(1, order + 1):
            f.write("ngram %d=%d\n" % (k, sum(len(g) == k for g in ngrams)))
        for k in range(1, order + 1):
            f.write("\n\\%d-grams:\n" % k)
            for g in sorted(g for g in ngrams if len(g) == k):
                lp, bo = ngrams[g]
                f.write("%r\t%s%s\n" % (lp, " ".join(names[w] for w in g), "" if bo is None else "\t%r" % bo))
        f.write("\n\\end\\\n")


def compose(P, lm, scale, unk_id=None):
    """The composed lattice of the contract as a raw lattice dict with orig_arc, state_s, state_h."""
    scale = float(scale)
    unigrams = set(int(lm.word[c]) for c in range(lm.child_begin[0], lm.child_begin[1]))
    pairs, pair_off = [[lm.start]] + [None] * (P.S - 1), [0, 1]
    out = dict(src=[], dst=[], word=[], graph=[], acoustic=[], orig_arc=[])
    for n in range(1, P.S):
        cands = []
        for a in range(P.in_off[n], P.in_off[n + 1]):
            u = int(P.src[a])
            for j, h in enumerate(pairs[u]):
                if n == P.S - 1:
                    cost, hn = lm.final(h), 0
                elif P.word[a] == 0:
                    cost, hn = 0.0, h
                else:
                    w = int(P.word_ids[P.word[a]])
                    cost, hn = lm.arc(h, w if w in unigrams else unk_id)
                g = np.float32(np.float64(P.graph[a]) + scale * cost)
                cands.append((hn, len(cands), a, pair_off[u] + j, g))
        cands.sort(key=lambda c: (c[0], c[1]))
        pairs[n] = sorted(set(c[0] for c in cands))
        rank = {h: i for i, h in enumerate(pairs[n])}
        for hn, _, a, sp, g in cands:
            out["src"].append(sp); out["dst"].append(pair_off[n] + rank[hn]); out["word"].append(int(P.word_ids[P.word[a]]))
            out["graph"].append(g); out["acoustic"].append(P.acoustic[a]); out["orig_arc"].append(a)
        pair_off.append(pair_off[n] + len(pairs[n]))
    assert pairs[P.S - 1] == [0]
    n = pair_off[-1]
    final = np.full(n, np.inf, np.float32)
    final[n - 1] = 0.0
    return dict(num_states=n, start=0, src=np.asarray(out["src"], np.int32), dst=np.asarray(out["dst"], np.int32),
                word=np.asarray(out["word"], np.int32), graph=np.asarray(out["graph"], np.float32),
                acoustic=np.asarray(out["acoustic"], np.float32), orig_arc=np.asarray(out["orig_arc"], np.int64), final=final,
                state_s=np.repeat(np.arange(P.S), np.diff(pair_off)).astype(np.int32),
                state_h=np.asarray([h for ps in pairs for h in ps], np.int32))


def paths(num_states, start, src, dst, ends):
    """Every path from `start` to a state of `ends` as a tuple of arc indices."""
    outs = [[] for _ in range(num_states)]
    for a, s in enumerate(src):
        outs[int(s)].append(a)
    res, stack = [], [(start, ())]
    while stack:
        s, path = stack.pop()
        if s in ends:
            res.append(path)
        for a in outs[s]:
            stack.append((int(dst[a]), path + (a,)))
    return res


def same_composition(got, want):
    """None if the two composed dicts are equal in every integer and every float32 bit, else the first field that differs."""
    if int(got["num_states"]) != int(want["num_states"]):
        return "num_states %d != %d" % (got["num_states"], want["num_states"])
    for k in ("src", "dst", "word", "orig_arc", "state_s", "state_h"):
        if not np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)):
            return k
    for k in ("graph", "acoustic", "final"):
        if not np.array_equal(np.asarray(got[k], np.float32).view(np.uint32), np.asarray(want[k], np.float32).view(np.uint32)):
            return k
    return None
