"""Sequential restatement of the word-boundary alignment (pykaldi2_amd.score.WordLatticeBatch.align_words)
and a generator of utterances whose alignment is known by construction.  Plain Python: chain.split_to_phones cuts the
string into phones, the token and word rules are written out one phone at a time."""
import numpy as np

from pykaldi2_amd import chain
from pykaldi2_amd.lattice import TransitionModel
from pykaldi2_amd.score import WordBoundary

NONWORD, BEGIN, END, INTERNAL, SINGLETON = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- restatement
def tokens_of(cats):
    """[(first phone, last phone, kind)] with kind 0 silence, 1 word, 2 partial, from the phones' categories."""
    out, k, n = [], 0, len(cats)
    while k < n:
        e = k
        while e + 1 < n and not (cats[e + 1] in (NONWORD, SINGLETON, BEGIN) or cats[e] in (NONWORD, SINGLETON, END)):
            e += 1
        c = cats[k:e + 1]
        if len(c) == 1 and c[0] == NONWORD:
            kind = 0
        elif (len(c) == 1 and c[0] == SINGLETON) or (len(c) >= 2 and c[0] == BEGIN and c[-1] == END and
                                                      all(x == INTERNAL for x in c[1:-1])):
            kind = 1
        else:
            kind = 2
        out.append((k, e, kind))
        k = e + 1
    return out


def align_string(trans_model, word_boundary, tids, labels, path_times):
    """The record of align_words for one path: its string `tids`, its word labels and their arcs' own times."""
    ok, phones = chain.split_to_phones(trans_model, np.asarray(tids, np.int32)) if len(tids) else (True, [])
    cats = [word_boundary.category(p) for p, _, _ in phones]
    toks = tokens_of(cats)
    T = len(tids)
    span = lambda k, e: (phones[k][1], phones[e][1] + phones[e][2])
    words = [span(k, e) for k, e, kind in toks if kind != 0]
    reason = (0 if ok else 1) | (2 if any(kind == 2 for _, _, kind in toks) else 0) | (4 if len(words) != len(labels) else 0) | \
        (8 if 255 in cats else 0)
    assert not phones or phones[-1][1] + phones[-1][2] == T
    pt = np.asarray(path_times, np.int32).reshape(-1, 2)
    rec = dict(words=list(labels), path_times=pt, status=1 if reason else 0, reason=reason,
               phones=np.asarray(phones, np.int32).reshape(-1, 3))
    if reason:
        rec["times"], rec["silences"] = pt.copy(), np.zeros((0, 2), np.int32)
    else:
        rec["times"] = np.asarray(words, np.int32).reshape(-1, 2)
        rec["silences"] = np.asarray([span(k, e) for k, e, kind in toks if kind == 0], np.int32).reshape(-1, 2)
    return rec


def best_path_string(P, off, tids, backpointer):
    """(string, labels (global word ids), the word arcs' (begin, end)) of the path the back-pointers of a packed lattice
    describe; off / tids: packed_strings of the lattice."""
    arcs, s = [], P.S - 1
    while s > 0:
        a = int(backpointer[s])
        arcs.append(a)
        s = int(P.src[a])
    string, labels, times = [], [], []
    for a in reversed(arcs):
        piece = [int(x) for x in tids[off[a]:off[a + 1]]]
        if P.word[a] != 0:
            labels.append(int(P.word_ids[P.word[a]]))
            times.append((len(string), len(string) + len(piece)))
        string += piece
    return string, labels, times


def frame_capacity(P, arc_len):
    """The longest start -> end path of a packed lattice in frames, given the string length of every packed arc."""
    far = np.zeros(P.S, np.int64)
    for a in range(P.A):            # sorted by destination, every arc goes up a level: predecessors are complete
        far[P.dst[a]] = max(far[P.dst[a]], far[P.src[a]] + int(arc_len[a]))
    return int(far[-1])


def align_ref(batch, n, rec_post, trans_model, word_boundary):
    """The restatement on lattice n of a WordLatticeBatch whose strings are uploaded, for one record of arc_posteriors."""
    off, tids = batch.strings[n]
    return align_string(trans_model, word_boundary, *best_path_string(batch.packed[n], off, tids, rec_post["backpointer"]))


# ---------------------------------------------------------------- ground truth by construction
SIL = 1
TOPOLOGIES = ("bakis_reordered", "bakis", "chain")


class Model:
    """nb base phones x with the position-dependent variants x_B x_I x_E x_S and one silence phone; a transition model made
    with TransitionModel.from_topology: three-state Bakis (strings written reordered or not) or the one-state chain
    topology, in which a phone can last one frame."""

    def __init__(self, topology, nb=5):
        assert topology in TOPOLOGIES
        self.topology, self.nb = topology, nb
        self.reordered = topology != "bakis"
        self.ns = 1 if topology == "chain" else 3
        self.phones = [SIL] + [2 + 4 * b + v for b in range(nb) for v in range(4)]
        entry = [(s, s, [s, s + 1]) for s in range(self.ns)] + [(-1, -1, [])]
        tuples, pdf = [], 0
        for p in self.phones:
            for s in range(self.ns):
                tuples.append((p, s, pdf, pdf + 1 if topology == "chain" else pdf))
                pdf += 2
        self.trans_model = TransitionModel.from_topology({p: 0 for p in self.phones}, [entry], tuples)
        self.tid = {}                       # (phone, hmm state, self-loop?) -> transition-id
        t = 1
        for p, s, _, _ in tuples:
            self.tid[(p, s, True)], self.tid[(p, s, False)] = t, t + 1
            t += 2
        assert t == self.trans_model.num_transition_ids() + 1
        wb = {SIL: "nonword"}
        for b in range(nb):
            for v, name in enumerate(("begin", "internal", "end", "singleton")):
                wb[2 + 4 * b + v] = name
        self.word_boundary = WordBoundary(wb)

    def variant(self, base, v):
        return 2 + 4 * base + v

    def phone_string(self, phone, state_frames):
        """The transition-ids of one phone whose HMM state s lasts state_frames[s] >= 1 frames."""
        out = []
        for s, k in enumerate(state_frames):
            loops, fwd = [self.tid[(phone, s, True)]] * (k - 1), [self.tid[(phone, s, False)]]
            out += fwd + loops if self.reordered else loops + fwd
        return out


def make_utterance(rng, model, n_words, T=None, sil_prob=0.5, max_pron=3, extra="spread", vocab=50):
    """Draws words, pronunciations, optional silences and per-state durations.  T: the exact length in frames (None: random);
    extra: "spread" distributes the frames beyond one per HMM state at random, "one" gives them all to one state (one long
    self-loop run), "none" keeps every state at one frame (needs T = None).  Adjacent phones always differ, which keeps
    SplitToPhones' reordered detection unambiguous.  Returns dict(tids, labels, words [(label, begin, end)],
    silences [(begin, end)], phones [(phone, begin, duration)])."""
    units, last_base = [], -1             # (label or 0, [phones])
    if n_words == 0 or rng.random() < sil_prob:
        units.append((0, [SIL]))
    for w in range(n_words):
        L = int(rng.integers(1, max_pron + 1))
        bases = []
        for _ in range(L):
            b = int(rng.integers(0, model.nb))
            while b == last_base:
                b = int(rng.integers(0, model.nb))
            bases.append(b)
            last_base = b
        pron = [model.variant(bases[0], 3)] if L == 1 else \
            [model.variant(bases[0], 0)] + [model.variant(b, 1) for b in bases[1:-1]] + [model.variant(bases[-1], 2)]
        units.append((int(rng.integers(1, vocab + 1)), pron))
        if rng.random() < sil_prob:
            units.append((0, [SIL]))
            last_base = -1
    plist = [p for _, pron in units for p in pron]
    frames = np.ones((len(plist), model.ns), np.int64)
    if extra == "none":
        assert T is None
    else:
        more = int(rng.integers(0, 4 * frames.size + 1)) if T is None else T - frames.size
        assert more >= 0, "T = %r is below one frame per HMM state (%d)" % (T, frames.size)
        if extra == "one":
            frames[int(rng.integers(0, len(plist))), int(rng.integers(0, model.ns))] += more
        else:
            np.add.at(frames.reshape(-1), rng.integers(0, frames.size, more), 1)
    tids, words, sils, phones, labels, k = [], [], [], [], [], 0
    for label, pron in units:
        begin = len(tids)
        for p in pron:
            piece = model.phone_string(p, frames[k])
            phones.append((p, len(tids), len(piece)))
            tids += piece
            k += 1
        if label:
            words.append((label, begin, len(tids)))
            labels.append(label)
        else:
            sils.append((begin, len(tids)))
    assert T is None or len(tids) == T
    return dict(tids=tids, labels=labels, words=words, silences=sils, phones=phones)


def cut_path(rng, utt, n_empty=1, tail=True, labels=None):
    """Cuts an utterance's string into arcs at points that avoid the word boundaries where the string allows it, adds
    n_empty arcs with empty strings, keeps the tail of the string for the final weight and places every label on an arc of
    its own, in order -- before, on or after the arc that holds its phones.  Returns (pieces, arc labels, final string)."""
    tids, labels = utt["tids"], list(utt["labels"] if labels is None else labels)
    T, m = len(tids), len(labels)
    n_arcs = max(1, m + int(rng.integers(0, 3)))
    edges = {b for _, b, e in utt["words"]} | {e for _, b, e in utt["words"]}
    inner = [t for t in range(1, T) if t not in edges] or list(range(1, T))
    n_cuts = n_arcs - 1 + (1 if tail else 0)
    cuts = sorted(int(x) for x in rng.choice(inner, n_cuts, replace=False)) if len(inner) >= n_cuts else \
        sorted(int(x) for x in rng.integers(0, T + 1, n_cuts))
    bounds = [0] + cuts + [T]
    pieces = [tids[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)]
    final = pieces.pop() if tail else []
    for _ in range(n_empty):
        pieces.insert(int(rng.integers(0, len(pieces) + 1)), [])
    where = sorted(int(x) for x in rng.choice(len(pieces), m, replace=False)) if m else []
    arc_labels = [0] * len(pieces)
    for w, a in zip(labels, where):
        arc_labels[a] = w
    return pieces, arc_labels, final


def make_lattice(paths, decoy=True):
    """A raw lattice dict (the form pack_lattice accepts, with strings) of parallel chains from the start state, one per
    path = (pieces, arc labels, final string, graph cost, acoustic cost); the costs sit on the path's first arc.  decoy:
    two more paths of very high cost that part at the start state and meet again after 2 and after 4 frames, so the state
    times of the lattice are inconsistent (state_times and mbr(times=True) refuse it)."""
    src, dst, word, graph, acoustic, strs, finals = [], [], [], [], [], [], {}
    n = 1
    if decoy:
        src += [0, 0, 2, 1]; dst += [1, 2, 1, 3]; word += [900, 901, 0, 902]; graph += [1e4, 1e4, 0.0, 0.0]
        acoustic += [0.0] * 4; strs += [[1, 2], [1], [2, 1, 2], []]; finals[3] = [1]
        n = 4
    for pieces, arc_labels, final, g, c in paths:
        s = 0
        for i, (piece, w) in enumerate(zip(pieces, arc_labels)):
            src.append(s); dst.append(n); word.append(w); strs.append(list(piece))
            graph.append(g if i == 0 else 0.0); acoustic.append(c if i == 0 else 0.0)
            s, n = n, n + 1
        finals[s] = list(final)
    fin = np.full(n, np.inf, np.float32)
    fstrs = [[] for _ in range(n)]
    for s, f in finals.items():
        fin[s], fstrs[s] = 0.0, f
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    flat = lambda xs: np.asarray([t for x in xs for t in x], np.int32)
    return dict(num_states=n, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                word=np.asarray(word, np.int32), graph=np.asarray(graph, np.float32), acoustic=np.asarray(acoustic, np.float32),
                final=fin, final_acoustic=np.zeros(n, np.float32), tid_off=off(strs), tids=flat(strs),
                final_tid_off=off(fstrs), final_tids=flat(fstrs))


def truth_record(utt, pieces, arc_labels):
    """The record align_words must return for a well-formed utterance cut by cut_path."""
    begins = np.concatenate([[0], np.cumsum([len(x) for x in pieces])])
    pt = [(int(begins[a]), int(begins[a + 1])) for a, w in enumerate(arc_labels) if w]
    return dict(words=list(utt["labels"]), times=np.asarray([(b, e) for _, b, e in utt["words"]], np.int32).reshape(-1, 2),
                silences=np.asarray(utt["silences"], np.int32).reshape(-1, 2), path_times=np.asarray(pt, np.int32).reshape(-1, 2),
                phones=np.asarray(utt["phones"], np.int32).reshape(-1, 3), status=0, reason=0)


def same_record(a, b, phones=True):
    keys = ["words", "times", "silences", "path_times", "status", "reason"] + (["phones"] if phones else [])
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype and (x == y).all(), (k, x, y)
        else:
            assert x == y, (k, x, y)
