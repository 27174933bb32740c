"""Lattice scoring on the device: best path, minimum Bayes risk decoding with word confidences and
Levenshtein word errors for a whole sweep of (LM weight, word insertion penalty) settings in one call -- what the
reference's example/*/local/score*.sh hand to Kaldi (lattice-scale | lattice-add-penalty | lattice-best-path,
lattice-mbr-decode, utt_wer.py).  Packing is numpy on the host; the kernels are csrc/lattice_score.hip.

    batch = WordLatticeBatch([lat0, lat1, ...], "cuda")        # dicts of compact_lattice / determinize_lattice / an archive
    for (words, cost) in batch.best_path(sweep())[0]: ...
    rec = batch.mbr(sweep(), decode_mbr=True)[0][0]             # words, conf, risk, iterations, status
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_SETTINGS = 64        # PK2_WORDLAT_MAX_SETTINGS
MAX_POSITIONS = 1023     # PK2_WORDLAT_MAX_POSITIONS
MAX_BINS = 8             # PK2_WORDLAT_MAX_BINS
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
    every local word (ascending)."""
    __slots__ = ("S", "A", "W", "depth", "cap", "src", "dst", "word", "graph", "acoustic", "in_off", "out_off", "out_idx",
                 "level_off", "word_ids", "word_off", "word_arcs", "orig_arc")


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

    def __len__(self):
        return len(self.packed)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().pk2_wordlat_destroy(h)

    # ---- launches cut to the workspace budget ----
    def _chunks(self, G, bins, workspace_mb):
        budget = int(workspace_mb * (1 << 20))
        L, out, first = _lib.lib(), [], 0
        one = lambda f, k: int(L.pk2_wordlat_workspace_bytes(self._h, f, k, G, bins))
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

    def mbr(self, settings, decode_mbr=True, max_iter=10, bins=0, workspace_mb=4096):
        """[[record per setting] per lattice], record = dict(words, conf, risk, iterations, status[, bins]).  status: 0 ok,
        1 not converged within max_iter E-steps, 2 the next hypothesis would not fit the row capacity (in both cases the
        record is the last E-step's hypothesis with its own statistics), 3 empty or failed."""
        st = _settings_array(settings)
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
            raise ValueError("max_iter must be an integer >= 1, got %r" % (max_iter,))
        if isinstance(bins, bool) or int(bins) != bins or not 0 <= bins <= MAX_BINS:
            raise ValueError("bins must be an integer in 0..%d, got %r" % (MAX_BINS, bins))
        bins, max_iter = int(bins), int(max_iter)
        G, L, dev, res = st.shape[0], _lib.lib(), self.device, []
        with torch.cuda.device(dev):
            for first, count in self._chunks(G, bins, workspace_mb):
                B = _Bufs(dev)
                ws_bytes = int(L.pk2_wordlat_workspace_bytes(self._h, first, count, G, bins))
                work = B(ws_bytes // 8 + 1, torch.float64)
                ps = self.packed[first:first + count]
                stride = max(1, max((p.cap - 1) // 2 for p in ps))
                bstride = max(p.cap for p in ps)
                n = count * G
                words, nw, conf = B(n * stride, torch.int32), B(n, torch.int32), B(n * stride, torch.float64)
                risk, iters, status = B(n, torch.float64), B(n, torch.int32), B(n, torch.int32)
                bn = B(n, torch.int32) if bins else None
                bw = B(n * bstride * bins, torch.int32) if bins else None
                bv = B(n * bstride * bins, torch.float64) if bins else None
                _lib.check(L.pk2_wordlat_mbr(self._h, first, count, _lib.ptr(st), G, int(bool(decode_mbr)), max_iter, bins,
                                             _lib.ptr(work), ws_bytes, _lib.ptr(words), _lib.ptr(conf), stride, _lib.ptr(nw),
                                             _lib.ptr(risk), _lib.ptr(iters), _lib.ptr(status), _lib.ptr(bn), _lib.ptr(bw),
                                             _lib.ptr(bv), bstride, _lib.stream_ptr(dev)))
                hw, hn, hc, hr, hi, hs = (t.cpu().numpy() for t in (words, nw, conf, risk, iters, status))
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
                                 status=int(hs[k]))
                        if bins:
                            nb = int(hbn[k]) if hs[k] != 3 else 0
                            o = k * bstride * bins
                            r["bins"] = [[(int(hbw[o + j * bins + t]), float(hbv[o + j * bins + t])) for t in range(bins)
                                          if hbw[o + j * bins + t] >= 0] for j in range(nb)]
                        row.append(r)
                    res.append(row)
        return res


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
