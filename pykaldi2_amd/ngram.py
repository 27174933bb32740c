"""Backoff n-gram language models for lattice rescoring: ARPA text -> the trie tables that
score.rescore_lm composes with a word lattice on the device.  Semantics: Kaldi's ConstArpaLmDeterministicFst, restated.

    lm = NgramLM.from_arpa("lm.arpa", words_txt="graph/words.txt", unk="<unk>")
    cost, h = lm.arc(lm.start, word_id)          # -ln p(word | history) with backoff, next LM state

Node 0 is the empty history, then the unigrams in ascending word id, then the order-k n-grams sorted by (parent node,
word): the children of a node are a contiguous range sorted by word.  Per node: word, cost = float32(-ln10 log10 p),
backoff = float32(-ln10 log10 bo) (0 where absent), child_begin (N + 1 entries), bo_link = node of the longest proper
suffix that is a node, next_state = node of the longest suffix of at most order - 1 words (possibly the n-gram itself) that
has children.  An LM state is a node with children, or node 0."""
import ctypes as C
import math

import numpy as np

from . import _lib

MAX_ORDER = 8            # PK2_NGRAM_MAX_ORDER
_LN10 = math.log(10.0)


def read_words_txt(path):
    """words.txt -> {word: id}"""
    table = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) == 2:
                table[parts[0]] = int(parts[1])
    return table


class NgramLM:
    def __init__(self):
        raise TypeError("use NgramLM.from_arpa or NgramLM.from_ngrams")

    # ---- construction ----
    @classmethod
    def from_ngrams(cls, ngrams, bos_id, eos_id, order, unk_id=None, repair=False):
        """ngrams = {tuple of word ids: (log10 prob, log10 backoff or None)}."""
        if isinstance(order, bool) or int(order) != order or not 1 <= order <= MAX_ORDER:
            raise ValueError("n-gram order %r outside 1..%d" % (order, MAX_ORDER))
        order = int(order)
        lm = object.__new__(cls)
        lm.order, lm.bos_id, lm.eos_id, lm.unk_id, lm.skipped = order, int(bos_id), int(eos_id), unk_id, 0
        by_len = [[] for _ in range(order + 1)]
        for g in ngrams:
            g = tuple(int(w) for w in g)
            if not 1 <= len(g) <= order:
                raise ValueError("n-gram %r: length outside 1..%d" % (g, order))
            if min(g) < 0:
                raise ValueError("n-gram %r: negative word id" % (g,))
            by_len[len(g)].append(g)
        if (lm.eos_id,) not in ngrams:
            raise ValueError("the LM has no unigram for the end-of-sentence word (id %d)" % lm.eos_id)
        if (lm.bos_id,) not in ngrams:
            raise ValueError("the LM has no unigram for the begin-of-sentence word (id %d)" % lm.bos_id)
        node_of = {(): 0}
        grams, parent = [()], [0]
        lm.order_off = [0, 1]
        for k in range(1, order + 1):
            level = []
            for g in by_len[k]:
                p = node_of.get(g[:-1])
                if p is None:
                    if not repair:
                        raise ValueError("n-gram %r: its context %r is not an n-gram of the LM" % (g, g[:-1]))
                    lm.skipped += 1
                    continue
                level.append((p, g[-1], g))
            level.sort()
            for p, _, g in level:
                node_of[g] = len(grams)
                grams.append(g)
                parent.append(p)
            lm.order_off.append(len(grams))
        N = len(grams)
        lm.num_nodes = N
        lm.order_off = np.asarray(lm.order_off, np.int32)
        lm.word = np.zeros(N, np.int32)
        lm.cost, lm.backoff = np.zeros(N, np.float32), np.zeros(N, np.float32)
        lm.bo_link, lm.next_state = np.zeros(N, np.int32), np.zeros(N, np.int32)
        lm.child_begin = (1 + np.searchsorted(np.asarray(parent[1:], np.int64), np.arange(N + 1), side="left")).astype(np.int32)
        has_children = np.diff(lm.child_begin) > 0
        for i in range(1, N):
            g = grams[i]
            lp, bo = ngrams[g]
            lm.word[i] = g[-1]
            lm.cost[i] = np.float32(-_LN10 * float(lp))
            lm.backoff[i] = np.float32(-_LN10 * float(bo)) if bo is not None else np.float32(0)
            for j in range(1, len(g)):
                n = node_of.get(g[j:])
                if n is not None:
                    lm.bo_link[i] = n
                    break
            for j in range(1 if len(g) == order else 0, len(g)):
                n = node_of.get(g[j:])
                if n is not None and has_children[n]:
                    lm.next_state[i] = n
                    break
        if not (np.isfinite(lm.cost).all() and np.isfinite(lm.backoff).all()):
            raise ValueError("the LM holds a non-finite probability or backoff weight")
        lm.start = int(lm.next_state[node_of[(lm.bos_id,)]])
        lm._node_of = node_of
        lm._handles = {}
        return lm

    @classmethod
    def from_arpa(cls, path, symbols=None, words_txt=None, bos="<s>", eos="</s>", unk=None, repair=False):
        """ARPA text.  N-grams with a word outside the symbol table are skipped and counted in lm.skipped; <s> and </s>
        get ids above the table when it does not hold them."""
        if (symbols is None) == (words_txt is None):
            raise ValueError("from_arpa: give exactly one of symbols= and words_txt=")
        table = dict(symbols) if symbols is not None else read_words_txt(words_txt)
        top = max(list(table.values()) + [0])
        for w in (bos, eos):
            if w not in table:
                top += 1
                table[w] = top
        if unk is not None and unk not in table:
            raise ValueError("from_arpa: the unknown word %r is not in the symbol table" % unk)
        counts, ngrams, skipped, k = {}, {}, 0, 0
        with open(path) as f:
            for line in f:
                line = line.strip()
                if not line or line == "\\data\\":
                    continue
                if line == "\\end\\":
                    break
                if line.startswith("ngram ") and "=" in line and k == 0:
                    n, c = line[6:].split("=")
                    counts[int(n)] = int(c)
                    continue
                if line.startswith("\\") and line.endswith("-grams:"):
                    k = int(line[1:-7])
                    if not 1 <= k <= MAX_ORDER:
                        raise ValueError("%s: n-gram order %d outside 1..%d" % (path, k, MAX_ORDER))
                    continue
                if k == 0:
                    continue
                parts = line.split()
                if len(parts) not in (k + 1, k + 2):
                    raise ValueError("%s: malformed %d-gram line %r" % (path, k, line))
                ids = [table.get(w) for w in parts[1:k + 1]]
                if any(i is None for i in ids):
                    skipped += 1
                    continue
                ngrams[tuple(ids)] = (float(parts[0]), float(parts[k + 1]) if len(parts) == k + 2 else None)
        if not ngrams:
            raise ValueError("%s: no n-grams" % path)
        if max(list(counts) + [0]) > MAX_ORDER:
            raise ValueError("%s: n-gram order %d outside 1..%d" % (path, max(counts), MAX_ORDER))
        order = max(max(len(g) for g in ngrams), max(list(counts) + [1]))
        lm = cls.from_ngrams(ngrams, table[bos], table[eos], order, unk_id=table[unk] if unk is not None else None,
                             repair=repair)
        lm.skipped += skipped
        return lm

    # ---- the LM as a deterministic acceptor (host; float64 sums in the order of the device) ----
    def find_child(self, node, w):
        lo, hi = int(self.child_begin[node]), int(self.child_begin[node + 1])
        i = lo + int(np.searchsorted(self.word[lo:hi], w))
        return i if i < hi and self.word[i] == w else -1

    def has_word(self, w):
        return self.find_child(0, w) >= 0

    def arc(self, h, w):
        """(cost, next state) of word id w from LM state h."""
        acc, node = 0.0, int(h)
        for _ in range(self.order + 1):
            c = self.find_child(node, w)
            if c >= 0:
                return acc + float(self.cost[c]), int(self.next_state[c])
            if node == 0:
                break
            acc += float(self.backoff[node])
            node = int(self.bo_link[node])
        raise KeyError("word id %d has no unigram in the LM" % w)

    def final(self, h):
        return self.arc(h, self.eos_id)[0]

    def tables(self):
        return dict(word=self.word, cost=self.cost, backoff=self.backoff, child_begin=self.child_begin,
                    bo_link=self.bo_link, next_state=self.next_state)

    # ---- device copy (one per device, made on first use) ----
    def handle(self, device):
        import torch
        dev = torch.device(device)
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in self._handles:
            _lib.require_gpu()
            h = C.c_void_p()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().pk2_ngram_create(
                    self.num_nodes, self.order, _lib.ptr(self.order_off), _lib.ptr(self.word), _lib.ptr(self.cost),
                    _lib.ptr(self.backoff), _lib.ptr(self.child_begin), _lib.ptr(self.bo_link), _lib.ptr(self.next_state),
                    self.start, self.eos_id, _lib.stream_ptr(dev), C.byref(h)))
            self._handles[key] = h
        return self._handles[key]

    def __del__(self):
        hs, self._handles = getattr(self, "_handles", {}), {}
        for h in hs.values():
            try:
                _lib.lib().pk2_ngram_destroy(h)
            except Exception:       # interpreter shutdown
                pass
