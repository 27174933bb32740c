"""Lattice scoring on the device: best path, minimum Bayes risk decoding with word confidences and
Levenshtein word errors for a whole sweep of (LM weight, word insertion penalty) settings in one call -- what the
reference's example/*/local/score*.sh hand to Kaldi (lattice-scale | lattice-add-penalty | lattice-best-path,
lattice-mbr-decode, utt_wer.py).  Packing is numpy on the host; the kernels are csrc/lattice_score.hip.

    batch = WordLatticeBatch([lat0, lat1, ...], "cuda")        # dicts of compact_lattice / determinize_lattice / an archive
    for (words, cost) in batch.best_path(sweep())[0]: ...
    rec = batch.mbr(sweep(), decode_mbr=True)[0][0]             # words, conf, risk, iterations, status
    rec = batch.mbr(sweep(), times=True)[0][0]                  # + times, path_times (frames)
    lines = ctm_lines("utt1", rec, symbols, frame_shift=0.03)   # "<key> 1 <begin> <duration> <word> <confidence>"
    rec = batch.oracle(refs, skip_words=(unk_id,))[0]          # lattice-oracle: errors, ins, dele, sub, words, arcs (7.16)
    arc_frames, frames = lattice_depth(batch.packed[0])         # lattice-depth = arc_frames / frames
    rec = batch.align_words(sweep(), trans_model, WordBoundary.read("phones/word_boundary.int"))[0][0]   # DESIGN.md 7.18:
    #   words, cost, times (int32: every word's own begin and end), silences, path_times, status, reason[, phones]

N-gram LM rescoring (csrc/lattice_lmrescore.hip, pykaldi2_amd.ngram): the composition of the lattices with a
backoff LM, what local/lmrescore_const_arpa.sh hands to Kaldi's lattice-lmrescore and lattice-lmrescore-const-arpa.

    lats = rescore_lm(lats, [(old_lm, -1.0), (new_lm, 1.0)])    # raw lattice dicts; fold_finals(lat) for CompactLatticeWriter
    new = batch.rescore_lm(new_lm, 1.0)                         # a WordLatticeBatch again

MBR system combination (csrc/lattice_combine.hip): the recipes' score_combine.sh, lattice-combine followed by
lattice-mbr-decode, without building the union lattice.

    recs = combine([lats_blstm, lats_transformer], sweep(), weights=[0.6, 0.4])   # [[record per setting] per utterance]
    cb = CombinedBatch([sysA, sysB, sysC]); cb.mbr(sweep(), bins=3); cb.best_path(sweep())
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_SETTINGS = 64        # PK2_WORDLAT_MAX_SETTINGS
MAX_POSITIONS = 1023     # PK2_WORDLAT_MAX_POSITIONS
MAX_BINS = 8             # PK2_WORDLAT_MAX_BINS
ALIGN_CHUNK = 256        # kWaThreads: frames (and phones) the word-alignment kernel takes per pass
LMRESCORE_SORT_LDS = 4096  # PK2_LMRESCORE_SORT_LDS: candidate arcs of one state the rescoring kernel sorts in LDS
_DEBUG_GUARD = False     # tests: NaN / sentinel poisoned buffers with checked guard padding around every device buffer
_GUARD = 64


def sweep(min_lmwt=7, max_lmwt=17, word_ins_penalty=(0.0, 0.5, 1.0)):
    """The recipes' sweep: [(lm, am, wip, (LMWT, wip))] with lm = 1, am = 1 / LMWT, LMWT outer and the penalty inner."""
    if int(min_lmwt) != min_lmwt or int(max_lmwt) != max_lmwt or not 1 <= min_lmwt <= max_lmwt:
        raise ValueError("sweep: need integers 1 <= min_lmwt <= max_lmwt, got %r, %r" % (min_lmwt, max_lmwt))
    out = []
    for lmwt in range(int(min_lmwt), int(max_lmwt) + 1):
        for wip in word_ins_penalty:
            out.append((1.0, 1.0 / lmwt, float(wip), (lmwt, float(wip))))
    return out


def _settings_array(settings):
    s = [tuple(float(x) for x in st[:3]) for st in settings]
    if not 1 <= len(s) <= MAX_SETTINGS:
        raise ValueError("need 1..%d settings per call, got %d" % (MAX_SETTINGS, len(s)))
    a = np.asarray(s, np.float64).reshape(len(s), 3)
    if not np.isfinite(a).all():
        raise ValueError("settings must be finite (lm, am, wip) triples")
    return np.ascontiguousarray(a)


class PackedLattice:
    """One word lattice in the form the kernels and the restatement (tests/mbr_ref.py) share.  States 0..S-1 by (level, old
    id): 0 = start, S-1 = the single end; arcs sorted by (destination, original index): in_off is the CSR by destination,
    out_off / out_idx the CSR by source (arc indices ascending); level_off the state range of every level; word = local
    id (0 = epsilon, ascending word id <-> ascending local id), word_ids the global ids, word_off / word_arcs the arcs of
    every local word (ascending); arc_len the length in frames of every arc's transition-id string (None for a lattice
    form without strings), read only by state_times."""
    __slots__ = ("S", "A", "W", "depth", "cap", "src", "dst", "word", "graph", "acoustic", "in_off", "out_off", "out_idx",
                 "level_off", "word_ids", "word_off", "word_arcs", "orig_arc", "arc_len")


def _lattice_arcs(lat, name):
    """Any of the three accepted forms -> (num_states, start, src, dst, word, graph, acoustic, final graph, final acoustic)."""
    if "arcs" in lat and "finals" in lat:           # kaldi_io.read_compact_lattice_ark
        n = int(lat["num_states"])
        arcs = lat["arcs"]
        src = np.asarray([a[0] for a in arcs], np.int64)
        dst = np.asarray([a[1] for a in arcs], np.int64)
        word = np.asarray([a[3] for a in arcs], np.int64)
        g = np.asarray([a[4][0] for a in arcs], np.float32)
        c = np.asarray([a[4][1] for a in arcs], np.float32)
        fg = np.asarray([f[0] for f in lat["finals"]], np.float32).reshape(-1)
        fc = np.asarray([f[1] for f in lat["finals"]], np.float32).reshape(-1)
        fc = np.where(np.isfinite(fg), fc, np.float32(0))
    elif "src" in lat and "final" in lat:           # compact_lattice (raw) / determinize_lattice
        n = int(lat["num_states"])
        src, dst = np.asarray(lat["src"], np.int64), np.asarray(lat["dst"], np.int64)
        word = np.asarray(lat["word"], np.int64)
        g, c = np.asarray(lat["graph"], np.float32), np.asarray(lat["acoustic"], np.float32)
        fg = np.asarray(lat["final"], np.float32).reshape(-1)
        fc = np.asarray(lat["final_acoustic"], np.float32).reshape(-1) if "final_acoustic" in lat else np.zeros(n, np.float32)
        fc = np.where(np.isfinite(fg), fc, np.float32(0))
    else:
        raise ValueError("lattice %s: not a compact_lattice / determinize_lattice / archive dict" % name)
    if fg.shape[0] != n or not (src.shape == dst.shape == word.shape == g.shape == c.shape):
        raise ValueError("lattice %s: inconsistent array sizes" % name)
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n):
        raise ValueError("lattice %s: arc endpoint outside 0..%d" % (name, n - 1))
    if (word < 0).any():
        raise ValueError("lattice %s: negative word id" % name)
    if not (np.isfinite(g).all() and np.isfinite(c).all()):
        raise ValueError("lattice %s: non-finite arc cost" % name)
    return n, int(lat["start"]), src, dst, word, g, c, fg, fc


def _string_lengths(lat):
    """(length of the transition-id string of every input arc, of every state's final weight) as int64 arrays; None for a
    form without strings or with string arrays that do not fit its arcs."""
    if "arcs" in lat and "finals" in lat:
        return (np.fromiter((len(a[4][2]) for a in lat["arcs"]), np.int64, len(lat["arcs"])),
                np.fromiter((len(f[2]) for f in lat["finals"]), np.int64, len(lat["finals"])))
    n, A = int(lat["num_states"]), np.asarray(lat["src"]).size
    if "tid_off" in lat and "final_tid_off" in lat:
        al, fl = np.diff(np.asarray(lat["tid_off"], np.int64)), np.diff(np.asarray(lat["final_tid_off"], np.int64))
    elif "tid" in lat:
        al, fl = (np.asarray(lat["tid"]).reshape(-1) > 0).astype(np.int64), np.zeros(n, np.int64)
    else:
        return None
    return (al, fl) if al.size == A and fl.size == n else None


def _packed_arc_len(P, lat, fg):
    """The string length of every packed arc: the arcs that packing made of the finals (orig_arc >= number of arcs, in
    state order) carry the final weight's string."""
    lens = _string_lengths(lat)
    if lens is None:
        return None
    both = np.concatenate([lens[0], lens[1][np.flatnonzero(np.isfinite(fg))]])
    return np.ascontiguousarray(both[P.orig_arc].astype(np.int64))


def state_times(P, lat=None, name="?"):
    """The frame at which every packed state is reached (int32, P.S entries): t(0) = 0, t(n) = t(s_a) + len_a for every
    incoming arc a of n, with len_a the length of the arc's transition-id string.  The incoming arcs must agree (Kaldi's
    CompactLatticeStateTimes asserts the same; ValueError naming the lattice, the state and the two frames); only the end
    state takes the maximum, the utterance length.  `lat` is the dict P was packed from (None: the lengths P carries)."""
    lens = P.arc_len if lat is None else _packed_arc_len(P, lat, _lattice_arcs(lat, name)[7])
    if lens is None:
        raise ValueError("lattice %s: no transition-id strings (tid_off / tid / archive strings), so no times" % name)
    t = np.zeros(P.S, np.int64)
    for lev in range(1, P.depth + 1):
        s0, s1 = int(P.level_off[lev]), int(P.level_off[lev + 1])
        a0, a1 = int(P.in_off[s0]), int(P.in_off[s1])
        cand = t[P.src[a0:a1]] + lens[a0:a1]
        off = P.in_off[s0:s1].astype(np.int64) - a0
        hi, lo = np.maximum.reduceat(cand, off), np.minimum.reduceat(cand, off)
        bad = np.flatnonzero(hi != lo)
        if bad.size and s0 + int(bad[0]) != P.S - 1:
            raise ValueError("lattice %s: state %d is reached at frame %d and at frame %d: the transition-id strings of its "
                             "incoming arcs disagree" % (name, s0 + int(bad[0]), int(lo[bad[0]]), int(hi[bad[0]])))
        t[s0:s1] = hi
    if t[-1] >= 2 ** 31:
        raise ValueError("lattice %s: %d frames" % (name, int(t[-1])))
    return t.astype(np.int32)


def fix_word_times(times):
    """Kaldi's clean-up of one-best word times on a copy of `times` (rows of (begin, end), float64), left to right: a word
    that begins before its predecessor ends meets it half way (and the predecessor's begin stays <= its end); afterwards
    no word ends before it begins.  Rows of -1 (no time) are left alone and skipped as neighbours."""
    t = np.array(times, np.float64).reshape(-1, 2)
    prev = -1
    for i in range(t.shape[0]):
        if t[i, 0] < 0:
            continue
        if prev >= 0 and t[i, 0] < t[prev, 1]:
            m = 0.5 * (t[i, 0] + t[prev, 1])
            t[prev, 1] = t[i, 0] = m
            t[prev, 0] = min(t[prev, 0], t[prev, 1])
        prev = i
    ok = t[:, 0] >= 0
    t[ok, 1] = np.maximum(t[ok, 1], t[ok, 0])
    return t


def ctm_lines(key, rec, symbols, frame_shift=0.01, channel="1", drop=("<UNK>",), times_key="times"):
    """The CTM lines of a record of mbr(times=True): "<key> <channel> <begin> <duration> <word> <confidence>", seconds with
    three decimals from fix_word_times(rec["times"]); symbols: word id -> symbol.  Symbols in `drop` and words without a
    time are left out.  times_key names the record's entry to print; integer times (align_words: every word's own begin
    and end, which cannot overlap) are printed as they are, without fix_word_times."""
    t = np.asarray(rec[times_key])
    t = t.reshape(-1, 2).astype(np.float64) if np.issubdtype(t.dtype, np.integer) else fix_word_times(t)
    out = []
    for i, w in enumerate(rec["words"]):
        sym = symbols.get(w, str(w))
        if sym in drop or t[i, 0] < 0:
            continue
        out.append("%s %s %.3f %.3f %s %.4f" % (key, channel, t[i, 0] * frame_shift, (t[i, 1] - t[i, 0]) * frame_shift, sym,
                                                float(rec["conf"][i])))
    return out


WORD_BOUNDARY_CATEGORIES = {"nonword": 0, "begin": 1, "end": 2, "internal": 3, "singleton": 4}


class WordBoundary:
    """Kaldi's phones/word_boundary.int as a table: .table[phone] (uint8) = 0 nonword, 1 begin, 2 end, 3 internal,
    4 singleton, 255 for a phone without an entry.  WordBoundary({phone: category}) or WordBoundary.read(path)."""

    def __init__(self, mapping):
        items = [(int(p), c) for p, c in dict(mapping).items()]
        for p, c in items:
            if p < 0 or (c not in WORD_BOUNDARY_CATEGORIES and c not in WORD_BOUNDARY_CATEGORIES.values()):
                raise ValueError("word boundary: phone %r with category %r" % (p, c))
        self.table = np.full(max([p for p, _ in items] + [0]) + 1, 255, np.uint8)
        for p, c in items:
            self.table[p] = WORD_BOUNDARY_CATEGORIES.get(c, c)

    @classmethod
    def read(cls, path):
        mapping = {}
        with open(path) as f:
            for n, line in enumerate(f, start=1):
                parts = line.split()
                if not parts:
                    continue
                ok = len(parts) == 2 and parts[0].isdigit() and parts[1] in WORD_BOUNDARY_CATEGORIES
                if not ok or int(parts[0]) in mapping:
                    raise ValueError("%s, line %d: expected `<phone-id> nonword|begin|end|internal|singleton`, one line per "
                                     "phone, got %r" % (path, n, line.rstrip("\n")))
                mapping[int(parts[0])] = parts[1]
        return cls(mapping)

    def category(self, phone):
        return int(self.table[phone]) if 0 <= phone < self.table.size else 255


def packed_strings(P, lat, name="?"):
    """(offsets int64 (P.A + 1), transition-ids int32) of the packed arcs of P, which was packed from the dict `lat`: the
    arcs that packing made of the finals (orig_arc >= number of arcs, in state order) carry the final weight's string; the
    one-tid form counts as strings of length 0 or 1.  ValueError for a lattice form without strings."""
    if _string_lengths(lat) is None:
        raise ValueError("lattice %s: no transition-id strings (tid_off / tid / archive strings), so no times" % name)
    astr, fstr = _strings(lat)
    fin = np.flatnonzero(np.isfinite(_lattice_arcs(lat, name)[7]))
    both = astr + [fstr[s] for s in fin]
    strs = [both[k] for k in P.orig_arc]
    off = np.concatenate([[0], np.cumsum([len(x) for x in strs])]).astype(np.int64)
    return off, np.asarray([t for x in strs for t in x], np.int32).reshape(-1)


class _AlignModel:
    """The device tables of pk2_wordalign_model_create for one (transition model, word boundary) pair."""

    def __init__(self, trans_model, word_boundary, device):
        if trans_model.tid2tstate is None or trans_model.tid_flags is None:
            raise ValueError("the transition model carries no topology (read it from final.mdl)")
        self.refs = (trans_model, word_boundary)
        h = C.c_void_p()
        cat = np.ascontiguousarray(word_boundary.table, np.uint8)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().pk2_wordalign_model_create(
                trans_model.num_transition_ids(), _lib.ptr(trans_model.tid2tstate), _lib.ptr(trans_model.tid2phone),
                _lib.ptr(trans_model.tid_flags), cat.size, _lib.ptr(cat), _lib.stream_ptr(device), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            _lib.lib().pk2_wordalign_model_destroy(h)


def _reach(n, start, frm, to):
    """States reachable from `start` along frm -> to."""
    order = np.argsort(frm, kind="stable")
    off = np.searchsorted(frm[order], np.arange(n + 1))
    nxt = to[order]
    seen = np.zeros(n, bool)
    seen[start] = True
    stack = [start]
    while stack:
        s = stack.pop()
        for t in nxt[off[s]:off[s + 1]]:
            if not seen[t]:
                seen[t] = True
                stack.append(int(t))
    return seen


def pack_lattice(lat, name="?"):
    """DESIGN.md 7.13 (host packing): finals -> epsilon arcs to one end state, trim, topological sort, levels, both CSR
    forms, local word ids.  ValueError naming the lattice for a cycle or no start -> end path."""
    n, start, src, dst, word, g, c, fg, fc = _lattice_arcs(lat, name)
    if not 0 <= start < max(n, 1) or n == 0:
        raise ValueError("lattice %s: empty (no start state)" % name)
    fin = np.flatnonzero(np.isfinite(fg))
    end = n
    src = np.concatenate([src, fin]).astype(np.int64)
    dst = np.concatenate([dst, np.full(fin.size, end)]).astype(np.int64)
    word = np.concatenate([word, np.zeros(fin.size, np.int64)])
    g = np.concatenate([g, fg[fin]]).astype(np.float32)
    c = np.concatenate([c, fc[fin]]).astype(np.float32)
    n += 1
    keep_state = _reach(n, start, src, dst) & _reach(n, end, dst, src)
    if not keep_state[end] or not keep_state[start]:
        raise ValueError("lattice %s: no path from the start state to a final state (%d states, %d arcs)"
                         % (name, n - 1, src.size - fin.size))
    keep = np.flatnonzero(keep_state[src] & keep_state[dst])          # original arc order survives
    src, dst, word, g, c = src[keep], dst[keep], word[keep], g[keep], c[keep]
    # Kahn: level = longest arc count from the start
    indeg = np.bincount(dst, minlength=n)
    order = np.argsort(src, kind="stable")
    off = np.searchsorted(src[order], np.arange(n + 1))
    nxt = dst[order]
    level = np.full(n, -1, np.int64)
    level[start] = 0
    if indeg[start] != 0:
        raise ValueError("lattice %s: cycle through the start state" % name)
    frontier, done = [start], 0
    while frontier:
        new = []
        for s in frontier:
            done += 1
            for t in nxt[off[s]:off[s + 1]]:
                level[t] = max(level[t], level[s] + 1)
                indeg[t] -= 1
                if indeg[t] == 0:
                    new.append(int(t))
        frontier = new
    if done != int(keep_state.sum()):
        raise ValueError("lattice %s: cycle (%d of %d states could be ordered)" % (name, done, int(keep_state.sum())))
    states = np.flatnonzero(keep_state)
    states = states[np.lexsort((states, level[states]))]              # by (level, old id)
    new_of = np.full(n, -1, np.int64)
    new_of[states] = np.arange(states.size)
    P = PackedLattice()
    P.S, P.A = int(states.size), int(src.size)
    s2, d2 = new_of[src], new_of[dst]
    by_dst = np.argsort(d2, kind="stable")
    P.src, P.dst = s2[by_dst].astype(np.int32), d2[by_dst].astype(np.int32)
    P.graph, P.acoustic = np.ascontiguousarray(g[by_dst]), np.ascontiguousarray(c[by_dst])
    P.orig_arc = keep[by_dst]                       # index into the input arcs, then the finals in state order
    w = word[by_dst]
    P.word_ids = np.unique(np.concatenate([[0], w])).astype(np.int32)
    P.word = np.searchsorted(P.word_ids, w).astype(np.int32)
    P.W = int(P.word_ids.size)
    P.in_off = np.searchsorted(P.dst, np.arange(P.S + 1)).astype(np.int32)
    P.out_idx = np.argsort(P.src, kind="stable").astype(np.int32)
    P.out_off = np.searchsorted(P.src[P.out_idx], np.arange(P.S + 1)).astype(np.int32)
    P.word_arcs = np.argsort(P.word, kind="stable").astype(np.int32)
    P.word_off = np.searchsorted(P.word[P.word_arcs], np.arange(P.W + 1)).astype(np.int32)
    lv = level[states]
    P.depth = int(lv[-1])
    P.level_off = np.searchsorted(lv, np.arange(P.depth + 2)).astype(np.int32)
    P.cap = min(MAX_POSITIONS, 2 * P.depth + 1)
    assert P.dst[-1] == P.S - 1 and P.level_off[1] == 1 and P.level_off[-1] - P.level_off[-2] == 1
    P.arc_len = _packed_arc_len(P, lat, fg)
    return P


def _alloc(shape, dtype, device):
    """Device buffer; under _DEBUG_GUARD poisoned (NaN / 0x7f7f7f7f) and surrounded by guard elements."""
    n = int(np.prod(shape)) if not isinstance(shape, int) else int(shape)
    if not _DEBUG_GUARD:
        return torch.empty(max(n, 1), dtype=dtype, device=device)[:n], None
    poison, guard = (float("nan"), -12345.0) if dtype.is_floating_point else (0x7f7f7f7f if dtype != torch.uint8 else 0x7f, 0x5a)
    whole = torch.full((n + 2 * _GUARD,), poison, dtype=dtype, device=device)
    whole[:_GUARD] = guard
    whole[_GUARD + n:] = guard
    return whole[_GUARD:_GUARD + n], (whole, n, guard)


def _check_guards(guards):
    for whole, n, guard in guards:
        if whole is None:
            continue
        h = whole.cpu()
        if not (bool((h[:_GUARD] == guard).all()) and bool((h[_GUARD + n:] == guard).all())):
            raise _lib.Pk2Error("lattice scoring wrote outside a buffer of %d x %s" % (n, whole.dtype))


class _Bufs:
    def __init__(self, device):
        self.device, self.guards = device, []

    def __call__(self, n, dtype):
        t, g = _alloc(n, dtype, self.device)
        if g is not None:
            self.guards.append(g)
        return t

    def check(self):
        _check_guards(self.guards)


class WordLatticeBatch:
    """Word lattices packed and uploaded once: one array per field for the whole batch, offsets per lattice."""

    def __init__(self, lattices, device="cuda", names=None):
        if len(lattices) == 0:
            raise ValueError("WordLatticeBatch: no lattices")
        names = list(names) if names is not None else [str(i) for i in range(len(lattices))]
        self.packed = [p if isinstance(p, PackedLattice) else pack_lattice(p, names[i]) for i, p in enumerate(lattices)]
        self.names = names
        self.source = [None if isinstance(p, PackedLattice) else p for p in lattices]
        self.device = torch.device(device)
        _lib.require_gpu()
        P = self.packed
        cat = lambda f, dt: np.ascontiguousarray(np.concatenate([getattr(p, f) for p in P]).astype(dt))
        cum = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)
        self._host = dict(
            state_off=cum([p.S for p in P]), arc_off=cum([p.A for p in P]), level_off_off=cum([p.depth + 2 for p in P]),
            word_off_off=cum([p.W + 1 for p in P]),
            src=cat("src", np.int32), dst=cat("dst", np.int32), word=cat("word", np.int32), graph=cat("graph", np.float32),
            acoustic=cat("acoustic", np.float32), in_off=cat("in_off", np.int32), out_off=cat("out_off", np.int32),
            out_idx=cat("out_idx", np.int32), level_off=cat("level_off", np.int32), word_ids=cat("word_ids", np.int32),
            word_off=cat("word_off", np.int32), word_arcs=cat("word_arcs", np.int32))
        h = C.c_void_p()
        H = self._host
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pk2_wordlat_create(
                len(P), _lib.ptr(H["state_off"]), _lib.ptr(H["arc_off"]), _lib.ptr(H["level_off_off"]),
                _lib.ptr(H["word_off_off"]), _lib.ptr(H["src"]), _lib.ptr(H["dst"]), _lib.ptr(H["word"]), _lib.ptr(H["graph"]),
                _lib.ptr(H["acoustic"]), _lib.ptr(H["in_off"]), _lib.ptr(H["out_off"]), _lib.ptr(H["out_idx"]),
                _lib.ptr(H["level_off"]), _lib.ptr(H["word_ids"]), _lib.ptr(H["word_off"]), _lib.ptr(H["word_arcs"]),
                _lib.stream_ptr(self.device), C.byref(h)))
        self._h = h
        self.state_time = None      # per lattice, once mbr(times=True) has asked for them
        self._labels = {}           # oracle(): the device arc labels per set of skipped words
        self.strings = self.frame_cap = None    # per lattice, once align_words has asked for them
        self._align_models = {}

    def _upload_times(self):
        """State times of every lattice (state_times; its ValueError surfaces here), uploaded once."""
        if self.state_time is not None:
            return
        ts = [state_times(p, None, self.names[i]) for i, p in enumerate(self.packed)]
        flat = np.ascontiguousarray(np.concatenate(ts).astype(np.int32))
        if flat.size != int(self._host["state_off"][-1]):
            raise ValueError("state times: %d entries for %d states" % (flat.size, int(self._host["state_off"][-1])))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pk2_wordlat_set_times(self._h, _lib.ptr(flat)))
        self.state_time = ts

    def __len__(self):
        return len(self.packed)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().pk2_wordlat_destroy(h)

    def rescore_lm(self, lm, scale=1.0, expand=8, max_expand=64):
        """This batch composed with an n-gram LM (ngram.NgramLM) at `scale`: a new WordLatticeBatch; the composed dicts
        are its .source."""
        return WordLatticeBatch(_rescore_batch(self, lm, float(scale), expand, max_expand), self.device, names=self.names)

    # ---- launches cut to the workspace budget ----
    def _chunks(self, G, bins, workspace_mb, times=False):
        budget = int(workspace_mb * (1 << 20))
        L, out, first = _lib.lib(), [], 0
        size = L.pk2_wordlat_times_workspace_bytes if times else L.pk2_wordlat_workspace_bytes
        one = lambda f, k: int(size(self._h, f, k, G, bins))
        while first < len(self.packed):
            count = 1
            if one(first, 1) > budget:
                p = self.packed[first]
                raise ValueError("lattice %d (%d states, %d arcs, %d words, depth %d) needs %d bytes of workspace for %d "
                                 "settings: more than workspace_mb=%d" % (first, p.S, p.A, p.W, p.depth, one(first, 1), G,
                                                                          workspace_mb))
            while first + count < len(self.packed) and one(first, count + 1) <= budget:
                count += 1
            out.append((first, count))
            first += count
        return out

    def _run_post(self, settings, want_post, workspace_mb=4096):
        st = _settings_array(settings)
        G, L, dev = st.shape[0], _lib.lib(), self.device
        H, res = self._host, []
        with torch.cuda.device(dev):
            for first, count in self._chunks(G, -1, workspace_mb):
                B = _Bufs(dev)
                ws_bytes = int(L.pk2_wordlat_workspace_bytes(self._h, first, count, G, -1))
                work = B(ws_bytes // 8 + 1, torch.float64)
                stride = max(1, max(p.depth for p in self.packed[first:first + count]))
                nS = int(H["state_off"][first + count] - H["state_off"][first])
                nA = int(H["arc_off"][first + count] - H["arc_off"][first])
                words, nw = B(count * G * stride, torch.int32), B(count * G, torch.int32)
                cost, aend, status = B(count * G, torch.float64), B(count * G, torch.float64), B(count * G, torch.int32)
                post = B(G * nA, torch.float64) if want_post else None
                bp = B(G * nS, torch.int32) if want_post else None
                _lib.check(L.pk2_wordlat_best_path(self._h, first, count, _lib.ptr(st), G, _lib.ptr(work), ws_bytes,
                                                   _lib.ptr(words), stride, _lib.ptr(nw), _lib.ptr(cost), _lib.ptr(aend),
                                                   _lib.ptr(post), _lib.ptr(bp), _lib.ptr(status), _lib.stream_ptr(dev)))
                hw, hn, hc, ha, hs = (t.cpu().numpy() for t in (words, nw, cost, aend, status))
                hp = post.cpu().numpy() if want_post else None
                hb = bp.cpu().numpy() if want_post else None
                B.check()
                for i in range(count):
                    p, row = self.packed[first + i], []
                    ao = G * int(H["arc_off"][first + i] - H["arc_off"][first])
                    so = G * int(H["state_off"][first + i] - H["state_off"][first])
                    for g_ in range(G):
                        k = i * G + g_
                        r = dict(words=[int(x) for x in hw[k * stride:k * stride + hn[k]]] if hs[k] == 0 else [],
                                 cost=float(hc[k]), alpha_end=float(ha[k]), status=int(hs[k]))
                        if want_post:
                            r["post"] = hp[ao + g_ * p.A:ao + (g_ + 1) * p.A].copy()
                            r["backpointer"] = hb[so + g_ * p.S:so + (g_ + 1) * p.S].copy()
                        row.append(r)
                    res.append(row)
        return res

    def best_path(self, settings, workspace_mb=4096):
        """[[(words, cost) per setting] per lattice]: the tropical best path under cost = lm graph + am acoustic + wip per word."""
        return [[(r["words"], r["cost"]) for r in row] for row in self._run_post(settings, False, workspace_mb)]

    def arc_posteriors(self, settings, workspace_mb=4096):
        """[[dict(alpha_end, post, backpointer, words, cost) per setting] per lattice]; post / backpointer are indexed by the
        PACKED arcs / states (self.packed[n])."""
        return self._run_post(settings, True, workspace_mb)

    def mbr(self, settings, decode_mbr=True, max_iter=10, bins=0, workspace_mb=4096, times=False):
        """[[record per setting] per lattice], record = dict(words, conf, risk, iterations, status[, bins]).  status: 0 ok,
        1 not converged within max_iter E-steps, 2 the next hypothesis would not fit the row capacity (in both cases the
        record is the last E-step's hypothesis with its own statistics), 3 empty or failed.
        times=True: the records gain `times` (float64 (m, 2): begin and end of every word in frames, raw:
        fix_word_times cleans them up; -1 without a time), `path_times` (int32 (m0, 2): the best path's own word arcs)
        and with bins `bin_times` (a (begin, end) per entry of `bins`; (-1, -1) for epsilon).  The state times are
        computed and uploaded on the first such call; a lattice whose strings disagree raises ValueError there."""
        st = _settings_array(settings)
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
            raise ValueError("max_iter must be an integer >= 1, got %r" % (max_iter,))
        if isinstance(bins, bool) or int(bins) != bins or not 0 <= bins <= MAX_BINS:
            raise ValueError("bins must be an integer in 0..%d, got %r" % (MAX_BINS, bins))
        bins, max_iter = int(bins), int(max_iter)
        G, L, dev, res = st.shape[0], _lib.lib(), self.device, []
        if times:
            self._upload_times()
        with torch.cuda.device(dev):
            for first, count in self._chunks(G, bins, workspace_mb, times):
                B = _Bufs(dev)
                ws_bytes = int((L.pk2_wordlat_times_workspace_bytes if times else L.pk2_wordlat_workspace_bytes)(
                    self._h, first, count, G, bins))
                work = B(ws_bytes // 8 + 1, torch.float64)
                ps = self.packed[first:first + count]
                stride = max(1, max((p.cap - 1) // 2 for p in ps))
                bstride = max(p.cap for p in ps)
                pstride = max(1, max(p.depth for p in ps))
                n = count * G
                words, nw, conf = B(n * stride, torch.int32), B(n, torch.int32), B(n * stride, torch.float64)
                risk, iters, status = B(n, torch.float64), B(n, torch.int32), B(n, torch.int32)
                bn = B(n, torch.int32) if bins else None
                bw = B(n * bstride * bins, torch.int32) if bins else None
                bv = B(n * bstride * bins, torch.float64) if bins else None
                args = (self._h, first, count, _lib.ptr(st), G, int(bool(decode_mbr)), max_iter, bins, _lib.ptr(work), ws_bytes,
                        _lib.ptr(words), _lib.ptr(conf), stride, _lib.ptr(nw), _lib.ptr(risk), _lib.ptr(iters),
                        _lib.ptr(status), _lib.ptr(bn), _lib.ptr(bw), _lib.ptr(bv), bstride)
                if times:
                    tm, pt = B(n * stride * 2, torch.float64), B(n * pstride * 2, torch.int32)
                    bt = B(n * bstride * bins * 2, torch.float64) if bins else None
                    _lib.check(L.pk2_wordlat_mbr_times(*args, _lib.ptr(tm), _lib.ptr(bt), _lib.ptr(pt), pstride,
                                                       _lib.stream_ptr(dev)))
                else:
                    _lib.check(L.pk2_wordlat_mbr(*args, _lib.stream_ptr(dev)))
                hw, hn, hc, hr, hi, hs = (t.cpu().numpy() for t in (words, nw, conf, risk, iters, status))
                if bins:
                    hbn, hbw, hbv = bn.cpu().numpy(), bw.cpu().numpy(), bv.cpu().numpy()
                if times:
                    htm, hpt = tm.cpu().numpy().reshape(-1, 2), pt.cpu().numpy().reshape(-1, 2)
                    hbt = bt.cpu().numpy().reshape(-1, 2) if bins else None
                B.check()
                for i in range(count):
                    row = []
                    for g_ in range(G):
                        k = i * G + g_
                        m = int(hn[k]) if hs[k] != 3 else 0
                        r = dict(words=[int(x) for x in hw[k * stride:k * stride + m]],
                                 conf=hc[k * stride:k * stride + m].copy(), risk=float(hr[k]), iterations=int(hi[k]),
                                 status=int(hs[k]))
                        if bins:
                            nb = int(hbn[k]) if hs[k] != 3 else 0
                            o = k * bstride * bins
                            r["bins"] = [[(int(hbw[o + j * bins + t]), float(hbv[o + j * bins + t])) for t in range(bins)
                                          if hbw[o + j * bins + t] >= 0] for j in range(nb)]
                            if times:
                                r["bin_times"] = [[(float(hbt[o + j * bins + t, 0]), float(hbt[o + j * bins + t, 1]))
                                                   for t in range(bins) if hbw[o + j * bins + t] >= 0] for j in range(nb)]
                        if times:
                            r["times"] = htm[k * stride:k * stride + m].copy()
                            path = hpt[k * pstride:(k + 1) * pstride]
                            r["path_times"] = path[:int((path[:, 0] >= 0).sum())].copy()
                        row.append(r)
                    res.append(row)
        return res

    # ---- word-boundary alignment (csrc/lattice_align_words.hip) ----
    def _upload_strings(self):
        """The transition-id strings of the packed arcs (packed_strings; its ValueError surfaces here), built and uploaded
        the first time an alignment is asked for."""
        if self.frame_cap is not None:
            return
        offs, tids = [], []
        for i, p in enumerate(self.packed):
            if self.source[i] is None:
                raise ValueError("lattice %s: no transition-id strings (tid_off / tid / archive strings), so no times"
                                 % self.names[i])
            o, t = packed_strings(p, self.source[i], self.names[i])
            offs.append(o)
            tids.append(t)
        base = np.concatenate([[0], np.cumsum([t.size for t in tids])]).astype(np.int64)
        off = np.ascontiguousarray(np.concatenate([o[:-1] + base[i] for i, o in enumerate(offs)] + [base[-1:]]).astype(np.int64))
        flat = np.ascontiguousarray(np.concatenate(tids + [np.zeros(1, np.int32)]).astype(np.int32))
        cap = np.zeros(len(self.packed), np.int32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pk2_wordlat_set_strings(self._h, _lib.ptr(off), _lib.ptr(flat)))
            _lib.check(_lib.lib().pk2_wordlat_frame_capacity(self._h, _lib.ptr(cap)))
        self.strings = [(o, t) for o, t in zip(offs, tids)]
        self.frame_cap = [int(c) for c in cap]

    def _align_chunks(self, G, workspace_mb):
        budget = int(workspace_mb * (1 << 20))
        L, out, first = _lib.lib(), [], 0
        one = lambda f, k: int(L.pk2_wordlat_workspace_bytes(self._h, f, k, G, -1)) + \
            int(L.pk2_wordlat_align_workspace_bytes(self._h, f, k, G))
        while first < len(self.packed):
            count = 1
            if one(first, 1) > budget:
                raise ValueError("lattice %d needs %d bytes of workspace for %d settings: more than workspace_mb=%d"
                                 % (first, one(first, 1), G, workspace_mb))
            while first + count < len(self.packed) and one(first, count + 1) <= budget:
                count += 1
            out.append((first, count))
            first += count
        return out

    def align_words(self, settings, trans_model, word_boundary, phones=False, workspace_mb=4096):
        """[[record per setting] per lattice]: the best path with every word's own begin and end frame, what the recipes'
        lattice-1best | lattice-align-words | nbest-to-ctm print.  record = dict(words, cost, times (int32
        (m, 2)), silences (int32 (k, 2)), path_times (int32 (m, 2): the word arcs' own times), status, reason[, phones
        (int32 (n, 3): phone, begin, duration)]).  status 0: aligned; 1: the path's string is not a sequence of whole words
        with one label each (reason: 1 SplitToPhones not ok, 2 a partial word, 4 words and labels differ in number, 8 a phone
        without a category): times = path_times, silences empty; 3: no best path, everything empty.  trans_model must carry
        the topology (TransitionModel.read / from_topology), word_boundary is a WordBoundary."""
        st = _settings_array(settings)
        key = (id(trans_model), id(word_boundary))
        if key not in self._align_models:
            self._align_models[key] = _AlignModel(trans_model, word_boundary, self.device)
        model = self._align_models[key]
        self._upload_strings()
        G, L, dev, H, res = st.shape[0], _lib.lib(), self.device, self._host, []
        with torch.cuda.device(dev):
            for first, count in self._align_chunks(G, workspace_mb):
                B = _Bufs(dev)
                ws_bytes = int(L.pk2_wordlat_workspace_bytes(self._h, first, count, G, -1))
                aw_bytes = int(L.pk2_wordlat_align_workspace_bytes(self._h, first, count, G))
                work, awork = B(ws_bytes // 8 + 1, torch.float64), B(aw_bytes // 8 + 1, torch.float64)
                ps = self.packed[first:first + count]
                stride = max(1, max(p.depth for p in ps))
                fstride = max(1, max(self.frame_cap[first:first + count]))
                nS = int(H["state_off"][first + count] - H["state_off"][first])
                n = count * G
                words, nw = B(n * stride, torch.int32), B(n, torch.int32)
                cost, aend, bstat = B(n, torch.float64), B(n, torch.float64), B(n, torch.int32)
                bp = B(G * nS, torch.int32)
                pt, wt = B(n * stride * 2, torch.int32), B(n * stride * 2, torch.int32)
                tok, ntok = B(n * fstride * 4, torch.int32), B(n, torch.int32)
                pho = B(n * fstride * 3, torch.int32) if phones else None
                nph, status, reason = B(n, torch.int32), B(n, torch.int32), B(n, torch.int32)
                _lib.check(L.pk2_wordlat_best_path(self._h, first, count, _lib.ptr(st), G, _lib.ptr(work), ws_bytes,
                                                   _lib.ptr(words), stride, _lib.ptr(nw), _lib.ptr(cost), _lib.ptr(aend),
                                                   None, _lib.ptr(bp), _lib.ptr(bstat), _lib.stream_ptr(dev)))
                _lib.check(L.pk2_wordlat_align_words(self._h, model.h, first, count, G, _lib.ptr(bp), _lib.ptr(bstat),
                                                     _lib.ptr(awork), aw_bytes, _lib.ptr(pt), _lib.ptr(wt), stride, _lib.ptr(tok),
                                                     _lib.ptr(ntok), fstride, _lib.ptr(pho), _lib.ptr(nph), fstride,
                                                     _lib.ptr(status), _lib.ptr(reason), _lib.stream_ptr(dev)))
                hw, hn, hc, hs, hr, hnt, hnp = (t.cpu().numpy() for t in (words, nw, cost, status, reason, ntok, nph))
                hpt, hwt = pt.cpu().numpy().reshape(n, stride, 2), wt.cpu().numpy().reshape(n, stride, 2)
                htok = tok.cpu().numpy().reshape(n, fstride, 4)
                hpho = pho.cpu().numpy().reshape(n, fstride, 3) if phones else None
                B.check()
                for i in range(count):
                    row = []
                    for g_ in range(G):
                        k = i * G + g_
                        m = int(hn[k]) if hs[k] != 3 else 0
                        r = dict(words=[int(x) for x in hw[k * stride:k * stride + m]], cost=float(hc[k]),
                                 times=hwt[k, :m].copy(), path_times=hpt[k, :m].copy(), status=int(hs[k]), reason=int(hr[k]))
                        t = htok[k, :int(hnt[k])] if hs[k] == 0 else htok[k, :0]
                        sil = t[t[:, 3] == 0]
                        r["silences"] = np.stack([sil[:, 1], sil[:, 1] + sil[:, 2]], axis=1).astype(np.int32)
                        if phones:
                            r["phones"] = hpho[k, :int(hnp[k]) if hs[k] != 3 else 0].copy()
                        row.append(r)
                    res.append(row)
        return res

    # ---- lattice oracle (csrc/lattice_oracle.hip) ----
    def _arc_labels(self, skip_words):
        """arc_label of the whole batch on the device: the local word id of every packed arc, 0 for epsilon and for the
        words of skip_words (global ids); cached per skip set."""
        key = tuple(sorted({int(w) for w in skip_words}))
        if key not in self._labels:
            skip = np.asarray(key, np.int64)
            lab = [np.where(np.isin(p.word_ids, skip)[p.word], 0, p.word) for p in self.packed]
            self._labels[key] = _lib.h2d(np.ascontiguousarray(np.concatenate(lab).astype(np.int32)), self.device)
        return self._labels[key]

    def _oracle_chunks(self, ref_off, workspace_mb):
        budget = int(workspace_mb * (1 << 20))
        L, out, first = _lib.lib(), [], 0
        one = lambda f, k: int(L.pk2_wordlat_oracle_workspace_bytes(self._h, f, k, _lib.ptr(ref_off[f:f + k + 1])))
        while first < len(self.packed):
            count = 1
            if one(first, 1) > budget:
                p = self.packed[first]
                raise ValueError("lattice %d (%d states, depth %d) needs %d bytes of workspace for a reference of %d words: "
                                 "more than workspace_mb=%d" % (first, p.S, p.depth, one(first, 1),
                                                                int(ref_off[first + 1] - ref_off[first]), workspace_mb))
            while first + count < len(self.packed) and one(first, count + 1) <= budget:
                count += 1
            out.append((first, count))
            first += count
        return out

    def oracle(self, refs, skip_words=(), workspace_mb=4096):
        """Kaldi's lattice-oracle: [dict(errors, ins, dele, sub, words, arcs, status) per lattice] for refs = one sequence
        of global word ids per lattice.  errors = the smallest edit distance between the reference and any path of the
        lattice = ins + dele + sub; words = that path's words (global ids), arcs = its arcs as indices into the input
        lattice's arcs (the arcs packing made of the final weights are left out).  Arcs of the words in skip_words (global
        ids) cost nothing and are left out of `words`; a reference word in that set never matches.  status: 0 ok, 2 a
        reference of more than MAX_POSITIONS words (errors -1, nothing else).  Ties between paths and edit types are
        broken by the rule of tests/oracle_ref.py."""
        if len(refs) != len(self.packed):
            raise ValueError("oracle: %d references for %d lattices" % (len(refs), len(self.packed)))
        local = []
        for i, (p, r) in enumerate(zip(self.packed, refs)):
            r = np.asarray(r, np.int64).reshape(-1)
            if r.size and r.min() <= 0:
                raise ValueError("lattice %s: reference word %d (word ids start at 1)" % (self.names[i], int(r.min())))
            k = np.minimum(np.searchsorted(p.word_ids, r), p.W - 1)
            local.append(np.where(p.word_ids[k] == r, k, -1).astype(np.int32))
        ref_off = np.concatenate([[0], np.cumsum([r.size for r in local])]).astype(np.int64)
        flat = np.ascontiguousarray(np.concatenate(local + [np.full(1, -1, np.int32)]))
        L, dev, res = _lib.lib(), self.device, []
        with torch.cuda.device(dev):
            labels = self._arc_labels(skip_words)
            ref_dev = _lib.h2d(flat, dev)
            for first, count in self._oracle_chunks(ref_off, workspace_mb):
                B = _Bufs(dev)
                off_host = np.ascontiguousarray(ref_off[first:first + count + 1])
                off_dev = _lib.h2d(off_host, dev)
                ws_bytes = int(L.pk2_wordlat_oracle_workspace_bytes(self._h, first, count, _lib.ptr(off_host)))
                work = B(ws_bytes // 8 + 1, torch.float64)
                stride = max(1, max(p.depth for p in self.packed[first:first + count]))
                errors, counts, status = B(count, torch.int32), B(3 * count, torch.int32), B(count, torch.int32)
                words, nw = B(count * stride, torch.int32), B(count, torch.int32)
                path, npath = B(count * stride, torch.int32), B(count, torch.int32)
                _lib.check(L.pk2_wordlat_oracle(self._h, first, count, _lib.ptr(labels), _lib.ptr(ref_dev), _lib.ptr(off_dev),
                                                _lib.ptr(off_host), _lib.ptr(work), ws_bytes, _lib.ptr(errors), _lib.ptr(counts),
                                                _lib.ptr(words), stride, _lib.ptr(nw), _lib.ptr(path), stride, _lib.ptr(npath),
                                                _lib.ptr(status), _lib.stream_ptr(dev)))
                he, hc, hs, hw, hn, hp, hm = (t.cpu().numpy() for t in (errors, counts, status, words, nw, path, npath))
                B.check()
                for i in range(count):
                    p = self.packed[first + i]
                    if hs[i] == 3:
                        raise _lib.Pk2Error("lattice %s: the oracle walk failed" % self.names[first + i])
                    ok = hs[i] == 0
                    pa = hp[i * stride:i * stride + hm[i]] if ok else hp[:0]
                    res.append(dict(errors=int(he[i]), ins=int(hc[3 * i]) if ok else 0, dele=int(hc[3 * i + 1]) if ok else 0,
                                    sub=int(hc[3 * i + 2]) if ok else 0,
                                    words=[int(x) for x in hw[i * stride:i * stride + hn[i]]] if ok else [],
                                    arcs=[int(p.orig_arc[a]) for a in pa if p.dst[a] != p.S - 1],
                                    packed_arcs=[int(a) for a in pa], status=int(hs[i])))
        return res


# ---- MBR system combination (csrc/lattice_combine.hip) ----
MAX_SYSTEMS = 8           # PK2_WORDLAT_MAX_SYSTEMS
COMBINE_MAX_ITER = 100    # PK2_WORDLAT_COMBINE_MAX_ITER


def pack_groups(groups, weights):
    """The host side of a combination, no device needed: groups = [[PackedLattice per present system] per utterance],
    weights = the raw weights of the same systems.  Returns dict(group_off, wn, log_wn, uvoc_off, uvoc, map, cap) in the
    layout of pk2_wordlat_set_groups plus `vocab` (the ascending union of every group's word ids, 0 first) and `maps` (per
    lattice: union local id -> the lattice's local id, W for a word it does not have)."""
    group_off, wn, vocab, maps, cap = [0], [], [], [], []
    for ps, ws in zip(groups, weights):
        w = np.asarray(ws, np.float64).reshape(-1)
        if not 1 <= len(ps) <= MAX_SYSTEMS or w.size != len(ps):
            raise ValueError("a group holds 1..%d lattices with one weight each, got %d and %d" % (MAX_SYSTEMS, len(ps), w.size))
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError("the weights must be positive and finite, got %r" % (list(ws),))
        wn.append(w / w.sum())
        u = np.unique(np.concatenate([p.word_ids for p in ps])).astype(np.int32)
        vocab.append(u)
        for p in ps:
            k = np.minimum(np.searchsorted(p.word_ids, u), p.W - 1)
            maps.append(np.where(p.word_ids[k] == u, k, p.W).astype(np.int32))
        cap.append(min(MAX_POSITIONS, 2 * max(p.depth for p in ps) + 1))
        group_off.append(group_off[-1] + len(ps))
    wn = np.ascontiguousarray(np.concatenate(wn))
    return dict(group_off=np.asarray(group_off, np.int32), wn=wn, log_wn=np.log(wn),
                uvoc_off=np.concatenate([[0], np.cumsum([v.size for v in vocab])]).astype(np.int64),
                uvoc=np.ascontiguousarray(np.concatenate(vocab)), map=np.ascontiguousarray(np.concatenate(maps)),
                cap=cap, vocab=vocab, maps=maps)


class CombinedBatch:
    """The lattices that K systems made of the same utterances, for minimum Bayes risk decoding of their weighted union --
    the recipes' score_combine.sh (lattice-combine --lat-weights | lattice-mbr-decode).  systems = K lists, one entry per
    utterance: a lattice dict, a PackedLattice, or None where the system has no lattice for it (the weights are then
    renormalised over the systems that have one).  No union lattice is built: DESIGN.md 7.17."""

    def __init__(self, systems, device="cuda", names=None, weights=None):
        systems = [list(s) for s in systems]
        K = len(systems)
        if not 1 <= K <= MAX_SYSTEMS:
            raise ValueError("CombinedBatch: %d systems (1..%d)" % (K, MAX_SYSTEMS))
        U = len(systems[0])
        if U == 0 or any(len(s) != U for s in systems):
            raise ValueError("CombinedBatch: every system needs one entry per utterance (None for a missing lattice)")
        weights = [1.0] * K if weights is None else [float(w) for w in weights]
        if len(weights) != K:
            raise ValueError("CombinedBatch: %d weights for %d systems" % (len(weights), K))
        if not all(np.isfinite(w) and w > 0 for w in weights):
            raise ValueError("CombinedBatch: the weights must be positive and finite, got %r" % (weights,))
        self.names = list(names) if names is not None else [str(i) for i in range(U)]
        self.present = [[k for k in range(K) if systems[k][u] is not None] for u in range(U)]
        for u, pr in enumerate(self.present):
            if not pr:
                raise ValueError("CombinedBatch: utterance %s has a lattice in no system" % self.names[u])
        flat = [systems[k][u] for u in range(U) for k in self.present[u]]
        flat_names = ["%s[%d]" % (self.names[u], k) for u in range(U) for k in self.present[u]]
        self.batch = WordLatticeBatch(flat, device, names=flat_names)
        self.device, self.weights, self.K = self.batch.device, weights, K
        off = np.concatenate([[0], np.cumsum([len(pr) for pr in self.present])])
        self.groups = [self.batch.packed[off[u]:off[u + 1]] for u in range(U)]
        self.host = pack_groups(self.groups, [[weights[k] for k in pr] for pr in self.present])
        H = self.host
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pk2_wordlat_set_groups(self.batch._h, U, _lib.ptr(H["group_off"]), _lib.ptr(H["wn"]),
                                                          _lib.ptr(H["log_wn"]), _lib.ptr(H["uvoc_off"]), _lib.ptr(H["uvoc"]),
                                                          _lib.ptr(H["map"])))

    def __len__(self):
        return len(self.groups)

    def _chunks(self, G, bins, workspace_mb):
        budget = int(workspace_mb * (1 << 20))
        L, out, first = _lib.lib(), [], 0
        one = lambda f, k: int(L.pk2_wordlat_combine_workspace_bytes(self.batch._h, f, k, G, bins))
        while first < len(self.groups):
            count = 1
            if one(first, 1) > budget:
                raise ValueError("utterance %s (%d systems) needs %d bytes of workspace for %d settings: more than "
                                 "workspace_mb=%d" % (self.names[first], len(self.groups[first]), one(first, 1), G, workspace_mb))
            while first + count < len(self.groups) and one(first, count + 1) <= budget:
                count += 1
            out.append((first, count))
            first += count
        return out

    def mbr(self, settings, decode_mbr=True, max_iter=10, bins=0, workspace_mb=4096, times=False):
        """[[record per setting] per utterance]: the records of WordLatticeBatch.mbr (words, conf, risk, iterations,
        status[, bins]) of the weighted union plus `system`: the system whose best path was the first hypothesis (-1 with
        status 3: a system of the utterance has no path).  Launches are cut to the workspace budget by whole utterances."""
        if times:
            raise ValueError("CombinedBatch.mbr: word times of a combination are not built (times=True)")
        st = _settings_array(settings)
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= max_iter <= COMBINE_MAX_ITER:
            raise ValueError("max_iter must be an integer in 1..%d, got %r" % (COMBINE_MAX_ITER, max_iter))
        if isinstance(bins, bool) or int(bins) != bins or not 0 <= bins <= MAX_BINS:
            raise ValueError("bins must be an integer in 0..%d, got %r" % (MAX_BINS, bins))
        bins, max_iter = int(bins), int(max_iter)
        G, L, dev, res = st.shape[0], _lib.lib(), self.device, []
        with torch.cuda.device(dev):
            for first, count in self._chunks(G, bins, workspace_mb):
                B = _Bufs(dev)
                ws_bytes = int(L.pk2_wordlat_combine_workspace_bytes(self.batch._h, first, count, G, bins))
                work = B(ws_bytes // 8 + 1, torch.float64)
                caps = self.host["cap"][first:first + count]
                stride, bstride, n = max(1, max((c - 1) // 2 for c in caps)), max(caps), count * G
                words, nw, conf = B(n * stride, torch.int32), B(n, torch.int32), B(n * stride, torch.float64)
                risk, iters, status, system = B(n, torch.float64), B(n, torch.int32), B(n, torch.int32), B(n, torch.int32)
                bn = B(n, torch.int32) if bins else None
                bw = B(n * bstride * bins, torch.int32) if bins else None
                bv = B(n * bstride * bins, torch.float64) if bins else None
                _lib.check(L.pk2_wordlat_combine(self.batch._h, first, count, _lib.ptr(st), G, int(bool(decode_mbr)), max_iter,
                                                 bins, _lib.ptr(work), ws_bytes, _lib.ptr(words), _lib.ptr(conf), stride,
                                                 _lib.ptr(nw), _lib.ptr(risk), _lib.ptr(iters), _lib.ptr(status),
                                                 _lib.ptr(system), _lib.ptr(bn), _lib.ptr(bw), _lib.ptr(bv), bstride,
                                                 _lib.stream_ptr(dev)))
                hw, hn, hc, hr, hi, hs, hy = (t.cpu().numpy() for t in (words, nw, conf, risk, iters, status, system))
                if bins:
                    hbn, hbw, hbv = bn.cpu().numpy(), bw.cpu().numpy(), bv.cpu().numpy()
                B.check()
                for i in range(count):
                    row = []
                    for g_ in range(G):
                        k = i * G + g_
                        m = int(hn[k]) if hs[k] != 3 else 0
                        r = dict(words=[int(x) for x in hw[k * stride:k * stride + m]],
                                 conf=hc[k * stride:k * stride + m].copy(), risk=float(hr[k]), iterations=int(hi[k]),
                                 status=int(hs[k]), system=self.present[first + i][int(hy[k])] if hy[k] >= 0 else -1)
                        if bins:
                            nb = int(hbn[k]) if hs[k] != 3 else 0
                            o = k * bstride * bins
                            r["bins"] = [[(int(hbw[o + j * bins + t]), float(hbv[o + j * bins + t])) for t in range(bins)
                                          if hbw[o + j * bins + t] >= 0] for j in range(nb)]
                        row.append(r)
                    res.append(row)
        return res

    def best_path(self, settings, workspace_mb=4096):
        """[[(words, cost, system) per setting] per utterance]: the path of the highest normalised weight in the union, on the
        host from the systems' own best paths: the system minimising cost_k + alpha_k(end) - log wn_k (a later one on <
        only), its words and the cost of its path in its own lattice; ([], inf, -1) where a system has no path."""
        per, res, l = self.batch._run_post(settings, False, workspace_mb), [], 0
        for u, pr in enumerate(self.present):
            row = []
            for g_ in range(len(per[0])):
                pick, bs = -1, 0.0
                for j in range(len(pr)):
                    r = per[l + j][g_]
                    if r["status"] != 0:
                        pick = -1
                        break
                    s = (r["cost"] + r["alpha_end"]) - float(self.host["log_wn"][l + j])
                    if pick < 0 or s < bs:
                        pick, bs = j, s
                row.append((per[l + pick][g_]["words"], per[l + pick][g_]["cost"], pr[pick]) if pick >= 0 else ([], float("inf"), -1))
            res.append(row)
            l += len(pr)
        return res


def combine(systems, settings, weights=None, device="cuda", names=None, **kw):
    """CombinedBatch(systems, device, names, weights).mbr(settings, **kw) in one call."""
    return CombinedBatch(systems, device, names=names, weights=weights).mbr(settings, **kw)


def lattice_depth(P):
    """(sum of the arcs' lengths in frames, frames of the utterance) of a packed lattice -- their ratio is Kaldi's
    lattice-depth, the average number of arcs that cross a frame; None for a lattice form without transition-id strings."""
    if P.arc_len is None:
        return None
    return int(P.arc_len.sum()), int(state_times(P)[-1])


def oracle_wer(batch_results, refs):
    """(errors, reference words) over the records of WordLatticeBatch.oracle."""
    return sum(r["errors"] for r in batch_results), sum(len(r) for r in refs)


# ---- n-gram LM rescoring (csrc/lattice_lmrescore.hip) ----
_LM_STATE = np.dtype([("s", np.int32), ("h", np.int32)])
_LM_ARC = np.dtype([("src", np.int32), ("dst", np.int32), ("word", np.int32), ("orig", np.int32), ("graph", np.float32),
                    ("acoustic", np.float32)])


def _lm_words(batch, lm):
    """The LM's word id of every local word of the batch (laid out like word_ids): the word itself, `unk` for a word the LM
    has no unigram for when it was loaded with one, otherwise ValueError naming the word id and the lattice."""
    uni = lm.word[1:int(lm.order_off[2])]
    out = []
    for i, p in enumerate(batch.packed):
        w = p.word_ids.astype(np.int32).copy()
        missing = ~np.isin(w, uni)
        missing[0] = False
        if missing.any():
            if lm.unk_id is None:
                raise ValueError("lattice %s: word id %d has no unigram in the LM (load it with unk= to map such words)"
                                 % (batch.names[i], int(w[missing][0])))
            w[missing] = lm.unk_id
        out.append(w)
    return np.ascontiguousarray(np.concatenate(out))


def _lmrescore_launch(batch, first, count, lm, lm_word_dev, scale, expand):
    """One pk2_wordlat_lmrescore call -> [(status, states, arcs) per lattice] (host structured arrays)."""
    L, dev, H = _lib.lib(), batch.device, batch._host
    rooms = [(int(expand * p.S), int(expand * p.A)) for p in batch.packed[first:first + count]]
    nS, nA = sum(r[0] for r in rooms), sum(r[1] for r in rooms)
    ws_bytes = int(L.pk2_wordlat_lmrescore_workspace_bytes(batch._h, first, count, float(expand)))
    if ws_bytes == 0:
        raise ValueError("rescore_lm: expand=%r gives a lattice more than 2^29 states or arcs" % (expand,))
    B = _Bufs(dev)
    work = B(ws_bytes // 8 + 1, torch.float64)
    ons, ona, status = B(count, torch.int32), B(count, torch.int32), B(count, torch.int32)
    states, arcs = B(2 * nS, torch.int32), B(6 * nA, torch.int32)
    _lib.check(L.pk2_wordlat_lmrescore(batch._h, first, count, lm.handle(dev), _lib.ptr(lm_word_dev), float(scale), float(expand),
                                       _lib.ptr(work), ws_bytes, _lib.ptr(ons), _lib.ptr(ona), _lib.ptr(states), nS,
                                       _lib.ptr(arcs), nA, _lib.ptr(status), _lib.stream_ptr(dev)))
    hs, ha, hst, hns, hna = (x.cpu().numpy() for x in (states, arcs, status, ons, ona))
    B.check()
    hs, ha = hs.view(_LM_STATE), ha.view(_LM_ARC)
    out, so, ao = [], 0, 0
    for i, (rs, ra) in enumerate(rooms):
        ok = hst[i] == 0
        out.append((int(hst[i]), hs[so:so + hns[i]].copy() if ok else None, ha[ao:ao + hna[i]].copy() if ok else None))
        so, ao = so + rs, ao + ra
    return out


def _strings(lat):
    """(transition-id string per arc, per state's final weight) of any accepted lattice form; None where the form has none."""
    if lat is None:
        return None, None
    if "arcs" in lat and "finals" in lat:
        return [list(a[4][2]) for a in lat["arcs"]], [list(f[2]) for f in lat["finals"]]
    n = int(lat["num_states"])
    if "tid_off" in lat:
        to, ti = np.asarray(lat["tid_off"]), np.asarray(lat["tids"])
        fo, fi = np.asarray(lat["final_tid_off"]), np.asarray(lat["final_tids"])
        return ([[int(x) for x in ti[to[a]:to[a + 1]]] for a in range(to.size - 1)],
                [[int(x) for x in fi[fo[s]:fo[s + 1]]] for s in range(n)])
    if "tid" in lat:
        return [[int(x)] if int(x) > 0 else [] for x in lat["tid"]], [[] for _ in range(n)]
    return None, None


def _composed_dict(p, src_lat, states, arcs):
    """The kernel's output as a raw lattice dict (the form pack_lattice accepts) with orig_arc = the packed input arc;
    `input_arc` follows it back to src_lat (an arc index, or number of arcs + rank of the final state for the arc that a
    final weight became) and the transition-id strings are copied along it."""
    n = states.shape[0]
    final = np.full(n, np.inf, np.float32)
    final[n - 1] = 0.0
    orig = arcs["orig"].astype(np.int64)
    d = dict(num_states=n, start=0, src=arcs["src"].copy(), dst=arcs["dst"].copy(), word=arcs["word"].copy(),
             graph=arcs["graph"].copy(), acoustic=arcs["acoustic"].copy(), final=final, orig_arc=orig,
             state_s=states["s"].copy(), state_h=states["h"].copy(), input_arc=np.asarray(p.orig_arc, np.int64)[orig])
    astr, fstr = _strings(src_lat)
    if astr is not None:
        fin_states = np.flatnonzero(np.isfinite(_lattice_arcs(src_lat, "?")[7]))
        nA = len(astr)
        strs = [astr[k] if k < nA else fstr[fin_states[k - nA]] for k in d["input_arc"]]
        d["tid_off"] = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
        d["tids"] = np.asarray([x for s in strs for x in s], np.int32)
        d["final_acoustic"] = np.zeros(n, np.float32)
        d["final_tid_off"] = np.zeros(n + 1, np.int64)
        d["final_tids"] = np.zeros(0, np.int32)
    return d


def fold_finals(lat):
    """A composed lattice (single end state with final weight 0) in the form CompactLatticeWriter and Kaldi expect: the arcs
    into the end state become the final weights of their source states (graph, acoustic and transition-id string of the
    arc) and the end state is dropped.  orig_arc / input_arc are kept for the arcs; final_orig_arc / final_input_arc hold
    those of the arcs that became final weights (-1 elsewhere)."""
    n = int(lat["num_states"])
    end = n - 1
    fin = np.asarray(lat["final"], np.float32)
    if n < 2 or fin[end] != 0 or np.isfinite(fin[:end]).any() or (np.asarray(lat["src"]) == end).any():
        raise ValueError("fold_finals: not a composed lattice (the last state must be the only final one, weight 0, no arc out)")
    dst = np.asarray(lat["dst"])
    to_end = dst == end
    keep, fa = np.flatnonzero(~to_end), np.flatnonzero(to_end)
    fs = np.asarray(lat["src"])[fa]
    if np.unique(fs).size != fs.size:
        raise ValueError("fold_finals: a state with two arcs into the end state")
    out = dict(num_states=end, start=int(lat["start"]))
    for k in ("src", "dst", "word", "graph", "acoustic"):
        out[k] = np.asarray(lat[k])[keep].copy()
    final, final_ac = np.full(end, np.inf, np.float32), np.zeros(end, np.float32)
    final[fs], final_ac[fs] = np.asarray(lat["graph"])[fa], np.asarray(lat["acoustic"])[fa]
    out["final"], out["final_acoustic"] = final, final_ac
    for k in ("orig_arc", "input_arc"):
        if k in lat:
            out[k] = np.asarray(lat[k])[keep].copy()
            f = np.full(end, -1, np.int64)
            f[fs] = np.asarray(lat[k])[fa]
            out["final_" + k] = f
    to = np.asarray(lat["tid_off"]) if "tid_off" in lat else np.zeros(dst.size + 1, np.int64)
    ti = np.asarray(lat["tids"]) if "tid_off" in lat else np.zeros(0, np.int32)
    strs = [ti[to[a]:to[a + 1]] for a in keep]
    out["tid_off"] = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
    out["tids"] = np.concatenate(strs + [np.zeros(0, np.int32)]).astype(np.int32)
    fstr = [np.zeros(0, np.int32)] * end
    for a, s in zip(fa, fs):
        fstr[s] = ti[to[a]:to[a + 1]]
    out["final_tid_off"] = np.concatenate([[0], np.cumsum([len(s) for s in fstr])]).astype(np.int64)
    out["final_tids"] = np.concatenate(fstr + [np.zeros(0, np.int32)]).astype(np.int32)
    return out


def _follow(prev, lat):
    """input_arc of `lat`, composed from the folded lattice `prev`, taken back to the lattice `prev` was composed from."""
    fin = np.flatnonzero(np.isfinite(np.asarray(prev["final"], np.float32)))
    back = np.concatenate([np.asarray(prev["input_arc"], np.int64), np.asarray(prev["final_input_arc"], np.int64)[fin]])
    lat["input_arc"] = back[lat["input_arc"]]


def _rescore_batch(batch, lm, scale, expand, max_expand):
    """The composed dict of every lattice of the batch; a lattice whose room was short is run again alone with twice the
    room, up to max_expand."""
    if not np.isfinite(scale):
        raise ValueError("rescore_lm: the LM scale must be finite, got %r" % (scale,))
    if not (np.isfinite(expand) and np.isfinite(max_expand) and 0 < expand <= max_expand):
        raise ValueError("rescore_lm: need 0 < expand <= max_expand, got %r, %r" % (expand, max_expand))
    dev = batch.device
    with torch.cuda.device(dev):
        lm_word_dev = _lib.h2d(_lm_words(batch, lm), dev)
        res = _lmrescore_launch(batch, 0, len(batch), lm, lm_word_dev, scale, expand)
        for i, p in enumerate(batch.packed):
            e = expand
            while res[i][0] == 2:
                e *= 2
                if e > max_expand:
                    raise ValueError("lattice %s (%d states, %d arcs): the lattice composed with the LM does not fit %g times "
                                     "its size (max_expand)" % (batch.names[i], p.S, p.A, max_expand))
                res[i] = _lmrescore_launch(batch, i, 1, lm, lm_word_dev, scale, e)[0]
            if res[i][0] != 0:
                raise _lib.Pk2Error("lattice %s: LM rescoring failed with status %d" % (batch.names[i], res[i][0]))
    return [_composed_dict(p, batch.source[i], res[i][1], res[i][2]) for i, p in enumerate(batch.packed)]


def rescore_lm(lattices, lms, device="cuda", expand=8, max_expand=64, names=None):
    """Composes every lattice with the LMs of lms = [(NgramLM, scale), ...] one after the other: [(old, -1.0), (new, 1.0)]
    takes the first-pass LM out and puts a larger one in (the recipes' lmrescore_const_arpa.sh).  Returns the composed
    lattices as raw dicts (single end state with final weight 0, `orig_arc` = the packed arc of the last composition's
    input, `input_arc` = the arc of the caller's lattice); fold_finals() turns one into the form of the archive writer.
    No determinisation follows (Kaldi determinises again; a determinised input stays deterministic on words)."""
    if len(lms) == 0:
        raise ValueError("rescore_lm: no LM")
    cur = list(lattices)
    for k, (lm, scale) in enumerate(lms):
        out = _rescore_batch(WordLatticeBatch(cur, device, names=names), lm, float(scale), expand, max_expand)
        if k > 0:
            for prev, lat in zip(cur, out):
                _follow(prev, lat)
        cur = [fold_finals(d) for d in out] if k + 1 < len(lms) else out
    return cur


def edit_distance(hyps, refs, device="cuda"):
    """Levenshtein distance (unit costs) of every (hypothesis, reference) pair of word-id sequences, on the device; a
    reference of at most 1023 words.  Returns an int32 array."""
    if len(hyps) != len(refs):
        raise ValueError("edit_distance: %d hypotheses for %d references" % (len(hyps), len(refs)))
    n = len(hyps)
    if n == 0:
        return np.zeros(0, np.int32)
    for r in refs:
        if len(r) > MAX_POSITIONS:
            raise ValueError("edit_distance: a reference of %d words (at most %d)" % (len(r), MAX_POSITIONS))
    if torch.device(device).type == "cpu":          # asked for by name (host-side tools and tests): the plain DP in numpy
        out = np.zeros(n, np.int32)
        for i, (x, y) in enumerate(zip(hyps, refs)):
            y = np.asarray(y, np.int64).reshape(-1)
            row = np.arange(y.size + 1)
            for xi in x:
                t = np.minimum(row[1:] + 1, row[:-1] + (y != xi))
                row = np.minimum.accumulate(np.concatenate([[row[0] + 1], t]) - np.arange(y.size + 1)) + np.arange(y.size + 1)
            out[i] = row[-1]
        return out
    flat = lambda seqs: np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32).reshape(-1) for s in seqs] + [np.zeros(1, np.int32)]))
    offs = lambda seqs: np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    dev = torch.device(device)
    _lib.require_gpu()
    with torch.cuda.device(dev):
        B = _Bufs(dev)
        hy, rf, ho, ro = (_lib.h2d(a, dev) for a in (flat(hyps), flat(refs), offs(hyps), offs(refs)))
        out = B(n, torch.int32)
        _lib.check(_lib.lib().pk2_edit_distance_batch(_lib.ptr(hy), _lib.ptr(ho), _lib.ptr(rf), _lib.ptr(ro), n, _lib.ptr(out),
                                                      _lib.stream_ptr(dev)))
        res = out.cpu().numpy().copy()
        B.check()
    return res


def wer(hyps, refs, device="cuda"):
    """(errors, reference words) over the pairs, as utt_wer.py counts them: an empty hypothesis costs len(ref)."""
    idx = [i for i in range(len(hyps)) if len(hyps[i]) > 0]
    errs = sum(len(refs[i]) for i in range(len(hyps)) if len(hyps[i]) == 0)
    if idx:
        errs += int(edit_distance([hyps[i] for i in idx], [refs[i] for i in idx], device).sum())
    return errs, sum(len(r) for r in refs)
