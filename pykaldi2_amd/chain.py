"""Host-side mirror of the ``kaldi.chain`` objects the reference's LF-MMI path uses
(reference bin/train_chain.py:184-202, ops/ops.py:243-280), backed by libpk2hip.so.

  DenominatorGraph(den_fst, num_pdfs)       bin/train_chain.py:167,202
  ChainTrainingOptions                       bin/train_chain.py:191-193
  SupervisionOptions                         bin/train_chain.py:184-188
  Supervision                                bin/train_chain.py:271-272
  MappedAligner.to_phone_alignment           bin/train_chain.py:195-200,263
  MappedAligner.align / align_batch          bin/train_se2.py:192-199,263
  alignment_to_proto_supervision             bin/train_chain.py:271
  proto_supervision_to_supervision           bin/train_chain.py:272
  compute_chain_objf_and_deriv(...)          ops/ops.py:265
  GraphSupervision / graph_supervisions      alignment-free LF-MMI (no counterpart in the reference): the numerator is
                                             the full sum over the training graph of the transcript

``den_fst`` may be a path to an OpenFst binary ``den.fst`` or a dict of arc
arrays (``num_states, start, src, dst, pdf, prob`` as produced by
pykaldi2_amd.synth.den_graph_arcs).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class ChainTrainingOptions:
    """kaldi.chain.ChainTrainingOptions (fields used by the reference)."""

    def __init__(self, leaky_hmm_coefficient=1.0e-05, xent_regularize=0.0, l2_regularize=0.0):
        self.leaky_hmm_coefficient = leaky_hmm_coefficient
        self.xent_regularize = xent_regularize
        self.l2_regularize = l2_regularize


class SupervisionOptions:
    """kaldi.chain.SupervisionOptions (reference bin/train_chain.py:184-188)."""

    def __init__(self):
        self.convert_to_pdfs = True
        self.frame_subsampling_factor = 3
        self.left_tolerance = 5
        self.right_tolerance = 5


class DenominatorGraph:
    def __init__(self, den_fst, num_pdfs):
        L = _lib.lib()
        h = C.c_void_p()
        if isinstance(den_fst, (str, bytes)):
            path = den_fst.encode() if isinstance(den_fst, str) else den_fst
            _lib.check(L.pk2_den_graph_from_openfst(path, int(num_pdfs), C.byref(h)))
        else:
            src = np.ascontiguousarray(den_fst["src"], dtype=np.int32)
            dst = np.ascontiguousarray(den_fst["dst"], dtype=np.int32)
            pdf = np.ascontiguousarray(den_fst["pdf"], dtype=np.int32)
            prob = np.ascontiguousarray(den_fst["prob"], dtype=np.float32)
            _lib.check(L.pk2_den_graph_create(int(den_fst["num_states"]), int(num_pdfs), src.shape[0],
                                              _lib.ptr(src), _lib.ptr(dst), _lib.ptr(pdf), _lib.ptr(prob),
                                              int(den_fst.get("start", 0)), C.byref(h)))
        self._h = h
        s, p, a = C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(L.pk2_den_graph_info(h, C.byref(s), C.byref(p), C.byref(a)))
        self._num_states, self._num_pdfs, self._num_arcs = s.value, p.value, a.value

    def num_states(self):
        return self._num_states

    def num_pdfs(self):
        return self._num_pdfs

    def num_arcs(self):
        return self._num_arcs

    def initial_probs(self):
        out = np.empty(self._num_states, dtype=np.float32)
        _lib.check(_lib.lib().pk2_den_graph_initial_probs(self._h, _lib.ptr(out)))
        return out

    def kernel_path(self, num_seqs):
        """0 = per-arc-pdf kernels, 1 = state-x kernels (a launch per frame), 2 = persistent recursion kernel."""
        return int(_lib.lib().pk2_den_graph_path(self._h, int(num_seqs)))

    def persist_form(self, num_seqs):
        """Form of the persistent kernel behind kernel_path() == 2: 2 = chunked table + streamed overflow
        (csrc/chain_den_persist2.hip); 0 = none.  (1 was the retired first kernel and is no longer returned.)"""
        return int(_lib.lib().pk2_den_graph_persist_form(self._h, int(num_seqs)))

    PLAN_FIELDS = ("family", "form", "NG", "need_fill", "xgather", "prep_merged", "tail_mergeable", "gamma_kernel")

    def plan(self, num_seqs, max_frames):
        """The route of a call on `num_seqs` sequences of at most `max_frames` frames (csrc/chain_internal.h: DenPlan), as a
        dict over PLAN_FIELDS: family 0 = per-arc-pdf / 1 = state-x kernels, form as persist_form(), gamma_kernel 1 = LDS
        row / 0 = gather; the rest are flags."""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(_lib.lib().pk2_den_graph_plan(self._h, int(num_seqs), int(max_frames), _lib.ptr(out)))
        pl = dict(zip(self.PLAN_FIELDS, (int(v) for v in out)))
        # what the persistent kernel copies into LDS per frame on THIS graph (csrc/chain_internal.h: kDirectDeg): entries of
        # the table prefix / of the whole vector, and the arcs that read the vector in L2 instead, per direction
        for name, which in (("fwd", 0), ("bwd", 1)):
            info = np.zeros(8, dtype=np.int32)
            _lib.check(_lib.lib().pk2_den_graph_debug_persist2_table(self._h, which, _lib.ptr(info), None, None, None))
            pl[name + "_table"] = (int(info[0]), int(info[1]))
            pl[name + "_direct_arcs"] = int(info[3])
        return pl

    def debug_persist2_table(self, which):
        """Table prefix of an ordering of the persistent layout (test hook; csrc/chain_internal.h: kDirectDeg): Rt, R, the
        position of every entry of the published vector and the direct-arc records [rank][record][thread]; None if the
        graph has no persistent layout.  Rt == R: the whole vector is the table."""
        L = _lib.lib()
        info = np.zeros(8, dtype=np.int32)
        _lib.check(L.pk2_den_graph_debug_persist2_table(self._h, which, _lib.ptr(info), None, None, None))
        if not info[1]:
            return None
        lay = self.debug_persist2(which)
        nr, nd, nt = lay["prob"].shape[0], int(info[5]), int(info[7])
        pos = np.empty(int(info[1]), np.int32)
        dprob, dpr = np.empty((nr, nd, nt), np.float32), np.empty((nr, nd, nt), np.uint32)
        _lib.check(L.pk2_den_graph_debug_persist2_table(self._h, which, _lib.ptr(info), _lib.ptr(pos), _lib.ptr(dprob), _lib.ptr(dpr)))
        return dict(Rt=int(info[0]), R=int(info[1]), table_entries=int(info[2]), direct_arcs=int(info[3]),
                    max_direct=int(info[4]), kDirect=nd, kDirectDeg=int(info[6]), pos=pos, dprob=dprob,
                    dpos=(dpr & 0xffff).astype(np.int64), drow=(dpr >> 16).astype(np.int64))

    def debug_persist2(self, which):
        """Persistent layout of an ordering (test hook; csrc/chain_internal.h: HostPersist2); None if absent."""
        L = _lib.lib()
        info = np.zeros(32, dtype=np.int32)
        _lib.check(L.pk2_den_graph_debug_persist2(self._h, which, _lib.ptr(info), *([None] * 17)))
        if not info[0]:
            return None
        R, T, K, W, SP, SEG = (int(v) for v in info[26:32])
        MC = SEG - 2
        pieces, rows = int(info[7]), int(info[9])
        out = dict(prob=np.empty((R, K, T), np.float32), idx2=np.empty((R, K // 2, T), np.uint32),
                   ends=np.empty((R, 2, T), np.uint32), first_row=np.empty((R, 2, T), np.int32),
                   uncovered=np.empty((R, 2), np.int32), ncomp=np.empty((R, 2), np.int32), rmap=np.empty((2, rows), np.int16),
                   pbeg=np.empty((R, MC + 1), np.int32),
                   sprob=np.empty((pieces, T, SP), np.float32), sidx2=np.empty((pieces, T, SP // 2), np.uint32),
                   sends=np.empty((pieces, T), np.uint32), sfirst_row=np.empty((R, MC, T), np.int32),
                   wcrow=np.empty((R, SEG, W), np.int32), row_begin=np.empty(R + 1, np.int32),
                   grp_begin=np.empty(R + 1, np.int32), row_leak=np.empty(rows, np.float32), row_psum=np.empty(rows, np.float32))
        order = ("prob", "idx2", "ends", "first_row", "uncovered", "ncomp", "rmap", "pbeg", "sprob", "sidx2", "sends", "sfirst_row", "wcrow",
                 "row_begin", "grp_begin", "row_leak", "row_psum")
        _lib.check(L.pk2_den_graph_debug_persist2(self._h, which, _lib.ptr(info), *[_lib.ptr(out[k]) for k in order]))
        out.update(estep=int(info[1]), K=int(info[2]), R=int(info[3]), tfloats=int(info[4]), max_rows=int(info[5]),
                   max_groups=int(info[6]), pieces=pieces, cap=int(info[8]), cbeg=[int(v) for v in info[10:10 + MC + 1]],
                   lds_off=[int(v) for v in info[20:20 + MC]], SP=SP, W=W, T=T, slots=K, row_arrays=int(info[19]))
        return out

    def debug_ordering(self, which):
        """Host-side work decomposition (test hook): which = 0 by dst, 1 by src, 2 by pdf (general kernels);
        3 = by virtual destination state, 4 = by src gathering virtual destination states (state-x kernels)."""
        L = _lib.lib()
        na, nc = C.c_int64(), C.c_int32()
        _lib.check(L.pk2_den_graph_debug_ordering(self._h, which, C.byref(na), C.byref(nc), None, None,
                                                  None, None, None, None))
        arcs = np.empty((na.value, 4), dtype=np.int32)
        k = int(L.pk2_den_graph_arcs_per_lane())
        meta = np.empty((na.value // k, 2), dtype=np.uint32)      # per lane {first chunk-local row, flush mask}
        wb_off = np.empty(nc.value + 1, dtype=np.int32)
        row0 = np.empty(nc.value, dtype=np.int32)
        nrows = np.empty(nc.value, dtype=np.int32)
        atomic = np.empty(nc.value, dtype=np.int32)
        _lib.check(L.pk2_den_graph_debug_ordering(self._h, which, None, None, _lib.ptr(arcs), _lib.ptr(meta),
                                                  _lib.ptr(wb_off), _lib.ptr(row0), _lib.ptr(nrows),
                                                  _lib.ptr(atomic)))
        out = dict(arcs=arcs, meta=meta, wb_off=wb_off, row0=row0, nrows=nrows, atomic=atomic, arcs_per_lane=k)
        if which >= 3:
            nv, nl, no = C.c_int32(), C.c_int64(), C.c_int32()
            _lib.check(L.pk2_den_graph_debug_virtual(self._h, which, C.byref(nv), None, None, None, None, None,
                                                     C.byref(nl), None, None, None, C.byref(no), None, None))
            S = self._num_states
            voff, ooff = np.empty(S + 1, dtype=np.int32), np.empty(S + 1, dtype=np.int32)
            vpdf, opdf = np.empty(nv.value, dtype=np.int32), np.empty(no.value, dtype=np.int32)
            real0, nreal, slot0 = (np.empty(nc.value, dtype=np.int32) for _ in range(3))
            leak = np.empty(nl.value, dtype=np.float32)
            loop_pdf, loop_prob = np.empty(S, dtype=np.int32), np.empty(S, dtype=np.float32)
            _lib.check(L.pk2_den_graph_debug_virtual(self._h, which, None, _lib.ptr(voff), _lib.ptr(vpdf),
                                                     _lib.ptr(real0), _lib.ptr(nreal), _lib.ptr(slot0), None,
                                                     _lib.ptr(leak), _lib.ptr(loop_pdf), _lib.ptr(loop_prob), None,
                                                     _lib.ptr(ooff), _lib.ptr(opdf)))
            out.update(voff=voff, vpdf=vpdf, real0=real0, nreal=nreal, slot0=slot0, row_leak=leak,
                       loop_pdf=loop_pdf, loop_prob=loop_prob, ooff=ooff, opdf=opdf)
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().pk2_den_graph_destroy(self._h)
                self._h = None
        except Exception:
            pass


class Supervision:
    """kaldi.chain.Supervision for one utterance (num_sequences = 1): an acyclic FST in which
    every arc consumes one frame and carries a pdf label.  Arrays (numpy, host):
    src/dst int32 (state 0 initial), pdf int32, weight f32 (-log prob), arcs sorted by the
    frame of their source state with frame_offsets[t] = first arc of frame t."""

    def __init__(self, fst, weight=1.0, label_dim=None):
        self.weight = float(weight)
        self.num_sequences = 1
        self.frames_per_sequence = int(fst["frames"])
        self.label_dim = label_dim
        self.num_states = int(fst["num_states"])
        self.src = np.ascontiguousarray(fst["src"], dtype=np.int32)
        self.dst = np.ascontiguousarray(fst["dst"], dtype=np.int32)
        self.pdf = np.ascontiguousarray(fst["pdf"], dtype=np.int32)
        self.arc_weight = np.ascontiguousarray(fst["weight"], dtype=np.float32)
        self.frame_offsets = np.ascontiguousarray(fst["frame_offsets"], dtype=np.int32)
        self.final_states = np.ascontiguousarray(fst["final_states"], dtype=np.int32)
        self.final_weights = np.ascontiguousarray(fst["final_weights"], dtype=np.float32)
        self.state_time = fst.get("state_time")
        assert self.frame_offsets.shape[0] == self.frames_per_sequence + 1


class ProtoSupervision:
    """kaldi.chain.ProtoSupervision: the phone sequence with durations and the tolerance options; the
    allowed-phone sets are produced (with the supervision) by pk2_supervision_create."""

    def __init__(self, opts, phones, durations):
        self.phones = np.ascontiguousarray(phones, dtype=np.int32)
        self.durations = np.ascontiguousarray(durations, dtype=np.int32)
        if self.phones.ndim != 1 or self.phones.shape != self.durations.shape or self.phones.shape[0] == 0:
            raise ValueError("phones and durations must be non-empty lists of equal length")
        self.frame_subsampling_factor = int(opts.frame_subsampling_factor)
        self.left_tolerance, self.right_tolerance = int(opts.left_tolerance), int(opts.right_tolerance)


def alignment_to_proto_supervision(opts, phones, durations):
    """kaldi.chain.alignment_to_proto_supervision (reference bin/train_chain.py:271)."""
    return ProtoSupervision(opts, phones, durations)


class _SupModel:
    """pk2_sup_model of a (tree, transition model) pair."""

    def __init__(self, tree, trans_model):
        if trans_model.entries is None:
            raise ValueError("the transition model carries no topology (read it from 0.trans_mdl / final.mdl)")
        max_phone = max(trans_model.phone2entry)
        p2e = np.full(max_phone + 1, -1, np.int32)
        for ph, e in trans_model.phone2entry.items():
            p2e[ph] = e
        e_off, fwd, loop, t_off, t_dst = [0], [], [], [0], []
        for states in trans_model.entries:
            for f, l, dsts in states:
                fwd.append(f); loop.append(l); t_dst.extend(dsts); t_off.append(len(t_dst))
            e_off.append(len(fwd))
        arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
        e_off, fwd, loop, t_off, t_dst = arr(e_off), arr(fwd), arr(loop), arr(t_off), arr(t_dst)
        tuples = arr(trans_model.tuples)
        L = _lib.lib()
        self._h = L.pk2_sup_model_create(max_phone, _lib.ptr(p2e), len(trans_model.entries), _lib.ptr(e_off),
                                         _lib.ptr(fwd), _lib.ptr(loop), _lib.ptr(t_off), _lib.ptr(t_dst),
                                         tuples.shape[0], _lib.ptr(tuples), tree.N, tree.P, tree.kind.shape[0],
                                         _lib.ptr(tree.kind), _lib.ptr(tree.key), _lib.ptr(tree.a), _lib.ptr(tree.b),
                                         tree.pool.shape[0], _lib.ptr(tree.pool))
        if not self._h:
            raise _lib.Pk2Error(L.pk2_last_error().decode())
        self.label_dim = trans_model.num_pdfs()

    def pdf(self, window, pdf_class):
        w = np.ascontiguousarray(window, dtype=np.int32)
        out = C.c_int32()
        _lib.check(_lib.lib().pk2_sup_model_pdf(self._h, _lib.ptr(w), int(pdf_class), C.byref(out)))
        return out.value

    def __del__(self):
        try:
            if self._h:
                _lib.lib().pk2_sup_model_destroy(self._h)
                self._h = None
        except Exception:
            pass


_sup_models = {}


def supervision_model(tree, trans_model):
    key = (id(tree), id(trans_model))
    hit = _sup_models.get(key)
    if hit is None or hit[0] is not tree or hit[1] is not trans_model:
        hit = _sup_models[key] = (tree, trans_model, _SupModel(tree, trans_model))
    return hit[2]


def proto_supervision_to_supervision(tree, trans_model, proto, convert_to_pdfs=True, with_allowed=False):
    """kaldi.chain.proto_supervision_to_supervision (reference bin/train_chain.py:272).  Raises when no path
    satisfies the time constraints (Kaldi returns false with a warning)."""
    if not convert_to_pdfs:
        raise NotImplementedError("only convert_to_pdfs=True (reference bin/train_chain.py:185) is built")
    m = supervision_model(tree, trans_model)
    L = _lib.lib()
    h = L.pk2_supervision_create(m._h, _lib.ptr(proto.phones), _lib.ptr(proto.durations), proto.phones.shape[0],
                                 proto.frame_subsampling_factor, proto.left_tolerance, proto.right_tolerance)
    if not h:
        raise _lib.Pk2Error(L.pk2_last_error().decode())
    try:
        n = [C.c_int32() for _ in range(5)]
        L.pk2_supervision_sizes(h, *[C.byref(v) for v in n])
        frames, ns, na, nf, nal = (v.value for v in n)
        src, dst, pdf = (np.empty(na, np.int32) for _ in range(3))
        w, foff, stime = np.empty(na, np.float32), np.empty(frames + 1, np.int32), np.empty(ns, np.int32)
        fin, finw = np.empty(nf, np.int32), np.empty(nf, np.float32)
        aoff = np.empty(frames + 1, np.int32) if with_allowed else None
        aph = np.empty(nal, np.int32) if with_allowed else None
        _lib.check(L.pk2_supervision_copy(h, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(pdf), _lib.ptr(w), _lib.ptr(foff),
                                          _lib.ptr(stime), _lib.ptr(fin), _lib.ptr(finw), _lib.ptr(aoff), _lib.ptr(aph)))
    finally:
        L.pk2_supervision_destroy(h)
    sup = Supervision(dict(num_states=ns, frames=frames, src=src, dst=dst, pdf=pdf, weight=w, frame_offsets=foff,
                           state_time=stime, final_states=fin, final_weights=finw), label_dim=m.label_dim)
    if with_allowed:
        sup.allowed_phones = [aph[aoff[t]:aoff[t + 1]].tolist() for t in range(frames)]
    return sup


def split_to_phones(trans_model, alignment):
    """Kaldi's SplitToPhones on a transition-id alignment -> (ok, [(phone, start, duration)])."""
    if trans_model.tid2tstate is None:
        raise ValueError("the transition model carries no topology (read it from final.mdl)")
    ali = np.ascontiguousarray(alignment, dtype=np.int32)
    T = ali.shape[0]
    phones, durs = np.empty(max(T, 1), np.int32), np.empty(max(T, 1), np.int32)
    n, ok = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().pk2_split_to_phones(_lib.ptr(trans_model.tid2tstate), _lib.ptr(trans_model.tid2phone),
                                              _lib.ptr(trans_model.tid_flags), trans_model.num_transition_ids(),
                                              _lib.ptr(ali), T, _lib.ptr(phones), _lib.ptr(durs), C.byref(n),
                                              C.byref(ok)))
    starts = np.concatenate([[0], np.cumsum(durs[:n.value])[:-1]]) if n.value else []
    return bool(ok.value), [(int(p), int(s), int(d)) for p, s, d in zip(phones[:n.value], starts, durs[:n.value])]


def supervision_from_alignment(aligner, tree, trans_model, opts, trans_ids):
    """The per-utterance block of reference bin/train_chain.py:262-272 as one call."""
    phone_ali = aligner.to_phone_alignment(trans_ids)
    proto = alignment_to_proto_supervision(opts, [item[0] for item in phone_ali], [item[2] for item in phone_ali])
    return proto_supervision_to_supervision(tree, trans_model, proto, opts.convert_to_pdfs)


def read_disambig(path):
    """phones/disambig.int: one integer per line (empty file or None -> [])."""
    if not path:
        return []
    with open(path) as f:
        return [int(tok) for line in f for tok in line.split()[:1]]


def read_symbols(path):
    """words.txt: `<word> <id>` per line -> {word: id}."""
    with open(path) as f:
        return {p[0]: int(p[1]) for p in (line.split() for line in f) if len(p) >= 2}


class Lexicon:
    """L.fst for the aligner (pk2_lexicon): a path to an OpenFst binary or a dict of arc arrays (num_states, start, src, dst,
    ilabel, olabel, weight, final; pykaldi2_amd.synth.lexicon_arcs).  Input labels in `disambig` count as epsilon."""

    def __init__(self, fst, disambig=()):
        L = _lib.lib()
        dis = np.ascontiguousarray(list(disambig), np.int32)
        if isinstance(fst, (str, bytes)):
            h = L.pk2_lexicon_from_openfst(fst.encode() if isinstance(fst, str) else fst, _lib.ptr(dis), dis.shape[0])
        else:
            a = {k: np.ascontiguousarray(fst[k], np.int32) for k in ("src", "dst", "ilabel", "olabel")}
            w = np.ascontiguousarray(fst["weight"], np.float32)
            fin = np.ascontiguousarray(fst["final"], np.float32)
            assert fin.shape[0] == int(fst["num_states"])
            h = L.pk2_lexicon_create(int(fst["num_states"]), int(fst.get("start", 0)), a["src"].shape[0], _lib.ptr(a["src"]),
                                     _lib.ptr(a["dst"]), _lib.ptr(a["ilabel"]), _lib.ptr(a["olabel"]), _lib.ptr(w), _lib.ptr(fin),
                                     _lib.ptr(dis), dis.shape[0])
        if not h:
            raise _lib.Pk2Error(L.pk2_last_error().decode())
        self._h = h

    def __del__(self):
        try:
            if self._h:
                _lib.lib().pk2_lexicon_destroy(self._h)
                self._h = None
        except Exception:
            pass


class AlignModel:
    """pk2_align_model: tree + transition model (topology, tuples, log_probs) + the two graph scales."""

    def __init__(self, tree, trans_model, transition_scale=1.0, self_loop_scale=1.0):
        lp = getattr(trans_model, "log_probs", None)
        if lp is None:
            raise ValueError("the transition model has no <LogProbs> (read it from final.mdl): the aligner needs them")
        if lp.shape[0] != trans_model.num_transition_ids() + 1:
            raise ValueError("<LogProbs> holds %d values for %d transition-ids" % (lp.shape[0], trans_model.num_transition_ids()))
        self._sup = _SupModel(tree, trans_model)      # keeps the tree / topology handle alive
        tuples = np.ascontiguousarray(trans_model.tuples, np.int32)
        lp = np.ascontiguousarray(lp, np.float64)
        L = _lib.lib()
        self._h = L.pk2_align_model_create(self._sup._h, tuples.shape[0], _lib.ptr(tuples), trans_model.num_transition_ids(),
                                           _lib.ptr(lp), float(transition_scale), float(self_loop_scale))
        if not self._h:
            raise _lib.Pk2Error(L.pk2_last_error().decode())

    def __del__(self):
        try:
            if self._h:
                _lib.lib().pk2_align_model_destroy(self._h)
                self._h = None
        except Exception:
            pass


ALIGN_OK, ALIGN_BEAM, ALIGN_NO_PATH, ALIGN_ERROR = 0, 1, 2, 3


class AlignmentGraphs:
    """Training graphs of a batch of transcripts (one pk2_align_compile call).  status[n]: 0 compiled, 2 no path of
    frames[n] frames, 3 error (errors[n] says why)."""

    def __init__(self, model, lexicon, texts, frames):
        word_off = np.cumsum([0] + [len(t) for t in texts]).astype(np.int32)
        words = np.ascontiguousarray([int(w) for t in texts for w in t] or [0], np.int32)
        self.frames = np.ascontiguousarray(frames, np.int32)
        assert self.frames.shape[0] == len(texts)
        L = _lib.lib()
        self._h = L.pk2_align_compile(model._h, lexicon._h, len(texts), _lib.ptr(word_off), _lib.ptr(words), _lib.ptr(self.frames))
        if not self._h:
            raise _lib.Pk2Error(L.pk2_last_error().decode())
        self._keep = (model, lexicon)
        self.n = len(texts)
        self.status, self.num_states, self.num_arcs, self.errors = [], [], [], []
        for i in range(self.n):
            v = [C.c_int32() for _ in range(3)]
            _lib.check(L.pk2_align_graphs_info(self._h, i, *[C.byref(x) for x in v]))
            self.status.append(v[0].value); self.num_states.append(v[1].value); self.num_arcs.append(v[2].value)
            self.errors.append(L.pk2_align_graphs_error(self._h, i).decode())

    def export(self, i):
        """Graph i as arrays: in_off[S+1], per in-arc src (-1 = from the start state), tid, pdf, weight (f32); final (f32)."""
        S, A = self.num_states[i], self.num_arcs[i]
        out = dict(in_off=np.empty(S + 1, np.int32), src=np.empty(A, np.int32), tid=np.empty(A, np.int32),
                   pdf=np.empty(A, np.int32), weight=np.empty(A, np.float32), final=np.empty(S, np.float32))
        _lib.check(_lib.lib().pk2_align_graphs_copy(self._h, i, *[_lib.ptr(out[k]) for k in
                                                                 ("in_off", "src", "tid", "pdf", "weight", "final")]))
        out["dst"] = np.repeat(np.arange(S, dtype=np.int32), np.diff(out["in_off"]))
        return out

    def workspace_bytes(self):
        return int(_lib.lib().pk2_align_workspace_bytes(self._h))

    def uses_lds(self):
        return bool(_lib.lib().pk2_align_use_lds(self._h))

    def to_device(self, device):
        """The packed batch in one pinned host-to-device copy."""
        L = _lib.lib()
        host = torch.empty(int(L.pk2_align_graphs_packed_words(self._h)), dtype=torch.int32).pin_memory()
        _lib.check(L.pk2_align_graphs_pack(self._h, _lib.ptr(host)))
        self._host = host
        return host.to(device, non_blocking=True)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().pk2_align_graphs_destroy(self._h)
                self._h = None
        except Exception:
            pass


_align_ws = {}


def align_viterbi(graphs, loglikes, acoustic_scale, beam):
    """One pk2_align_viterbi launch on the current stream.  loglikes: f32 device tensor [N, Tmax, P] (any row strides, unit
    column stride), prior already subtracted.  Returns device tensors (alignment i32[N, Tmax], costs f32[N, 3] = total,
    graph, acoustic, status i32[N])."""
    _lib.require_gpu()
    x = loglikes
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    N, Tmax, P = x.shape
    assert N == graphs.n and int(graphs.frames.max()) <= Tmax
    dev = graphs.to_device(x.device)
    key = x.device.index if x.device.index is not None else torch.cuda.current_device()
    need = graphs.workspace_bytes()
    ws = _align_ws.get(key)
    if ws is None or ws.numel() < need:      # grow-only
        _align_ws[key] = None
        ws = _align_ws[key] = torch.empty(int(need * 1.25) + 4096, dtype=torch.uint8, device=x.device)
    ali = torch.empty(N, Tmax, dtype=torch.int32, device=x.device)
    costs = torch.empty(N, 3, dtype=torch.float32, device=x.device)
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().pk2_align_viterbi(graphs._h, _lib.ptr(dev), _lib.ptr(x), x.stride(0), x.stride(1), P, Tmax,
                                            float(acoustic_scale), float(beam), _lib.ptr(ali), _lib.ptr(costs), _lib.ptr(status),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    ali._pk2_keepalive = (graphs, dev)
    return ali, costs, status


class MappedAligner:
    """kaldi.alignment.MappedAligner.  to_phone_alignment (reference bin/train_chain.py:195-200,263) splits the
    transition-ids of the label files into phones.  align / align_batch (reference bin/train_se2.py:192-199,263) make the
    transition-id alignment of a word transcript on the device: the training graph transcript x L.fst x tree x H is
    compiled on the host (csrc/align_graph.hip), the Viterbi pass aligns a whole minibatch in one launch
    (csrc/align_viterbi.hip).  The tree and L.fst of from_files are read at the first align."""

    _tree = _lexicon = _model = _symbols = _scaled_models = None
    _tree_path = _lexicon_path = _disambig_path = _symbols_path = None
    beam, retry_beam, transition_scale, self_loop_scale, acoustic_scale = 200.0, None, 1.0, 1.0, 0.1

    def __init__(self, trans_model):
        self.transition_model = trans_model

    @classmethod
    def from_files(cls, model_rxfilename, tree_rxfilename=None, lexicon_rxfilename=None, symbols_filename=None,
                   disambig_rxfilename=None, graph_compiler_opts=None, beam=200.0, transition_scale=1.0, self_loop_scale=1.0,
                   acoustic_scale=0.1, retry_beam=None, **unused):
        from .lattice import TransitionModel
        a = cls(TransitionModel.read(model_rxfilename))
        a._tree_path, a._lexicon_path = tree_rxfilename, lexicon_rxfilename
        a._disambig_path, a._symbols_path = disambig_rxfilename, symbols_filename
        a._set_options(beam, transition_scale, self_loop_scale, acoustic_scale, retry_beam)
        return a

    @classmethod
    def from_models(cls, trans_model, tree, lexicon, disambig=(), symbols=None, beam=200.0, transition_scale=1.0,
                    self_loop_scale=1.0, acoustic_scale=0.1, retry_beam=None):
        """Same as from_files with objects: tree = ContextDependency, lexicon = Lexicon / path / arc dict, symbols = {word: id}."""
        a = cls(trans_model)
        a._tree = tree
        a._lexicon = lexicon if isinstance(lexicon, Lexicon) else Lexicon(lexicon, disambig)
        a._symbols = symbols
        a._set_options(beam, transition_scale, self_loop_scale, acoustic_scale, retry_beam)
        return a

    def _set_options(self, beam, transition_scale, self_loop_scale, acoustic_scale, retry_beam):
        self.beam, self.transition_scale, self.self_loop_scale = float(beam), float(transition_scale), float(self_loop_scale)
        self.acoustic_scale, self.retry_beam = float(acoustic_scale), None if retry_beam is None else float(retry_beam)

    def to_phone_alignment(self, alignment, phones=None):
        """-> [(phone, start frame, duration)]."""
        return split_to_phones(self.transition_model, alignment)[1]

    def _graph_model(self):
        if self._model is None:
            if self._lexicon is None:
                if not self._lexicon_path:
                    raise RuntimeError("MappedAligner.align needs a lexicon: build the aligner with from_files(model, tree, "
                                       "L.fst, ...) or from_models")
                from .tree import ContextDependency
                if not self._tree_path:
                    raise RuntimeError("MappedAligner.align needs the tree")
                self._tree = ContextDependency.read(self._tree_path)
                self._lexicon = Lexicon(self._lexicon_path, read_disambig(self._disambig_path))
                if self._symbols_path:
                    self._symbols = read_symbols(self._symbols_path)
            self._model = AlignModel(self._tree, self.transition_model, self.transition_scale, self.self_loop_scale)
        return self._model, self._lexicon

    def _graph_model_scaled(self, transition_scale, self_loop_scale):
        """(AlignModel, Lexicon) with other graph scales than the aligner's own (graph_supervisions); built once per pair."""
        _, lexicon = self._graph_model()
        if self._scaled_models is None:
            self._scaled_models = {}
        key = (float(transition_scale), float(self_loop_scale))
        if key not in self._scaled_models:
            self._scaled_models[key] = AlignModel(self._tree, self.transition_model, *key)
        return self._scaled_models[key], lexicon

    def _words(self, text):
        if isinstance(text, str):
            text = text.split()
        out = []
        for w in text:
            if isinstance(w, str) and self._symbols is not None:
                if w not in self._symbols:
                    raise RuntimeError("word %r is not in the symbol table" % w)
                out.append(self._symbols[w])
            else:
                out.append(int(w))
        return out

    def compile(self, texts, frames):
        """Training graphs of transcripts for utterances of frames[n] frames (AlignmentGraphs)."""
        model, lexicon = self._graph_model()
        return AlignmentGraphs(model, lexicon, [self._words(t) for t in texts], frames)

    def _viterbi(self, x, lengths, texts, beam):
        graphs = self.compile(texts, lengths)
        ali, costs, status = align_viterbi(graphs, x, self.acoustic_scale, beam)
        return graphs, ali.cpu().numpy(), costs.cpu().numpy(), status.cpu().numpy()

    @staticmethod
    def _as_device(loglikes, dims):
        x = torch.from_numpy(np.ascontiguousarray(loglikes)) if isinstance(loglikes, np.ndarray) else loglikes
        if not x.is_cuda:
            _lib.require_gpu()
            x = x.to("cuda")
        x = x.detach().to(torch.float32)
        if x.dim() != dims:
            raise ValueError("log-likelihoods of shape %s, expected %d dimensions" % (tuple(x.shape), dims))
        return x if x.stride(-1) == 1 else x.contiguous()

    @staticmethod
    def _result(ali, cost, T):
        return {"alignment": [int(v) for v in ali[:T]], "likelihood": -float(cost[0]),
                "weight": (float(cost[1]), float(cost[2])), "best_path": None}

    def align(self, loglikes, text):
        """loglikes [T, P] (prior subtracted), text = word ids (list or whitespace string; words with a symbol table) ->
        {"alignment": [transition-ids], "likelihood": -cost, "weight": (graph cost, acoustic cost), "best_path": None}.
        Raises RuntimeError when the utterance cannot be aligned (after a retry at retry_beam, when set)."""
        self._graph_model()      # a missing lexicon / tree is reported before anything touches the device
        x = self._as_device(loglikes, 2)[None]
        T = int(x.shape[1])
        for beam in [self.beam] + ([self.retry_beam] if self.retry_beam else []):
            graphs, ali, costs, status = self._viterbi(x, [T], [text], beam)
            if status[0] == ALIGN_OK:
                return self._result(ali[0], costs[0], T)
            if status[0] != ALIGN_BEAM:
                break
        why = {ALIGN_BEAM: "no final state within the beam", ALIGN_NO_PATH: graphs.errors[0],
               ALIGN_ERROR: graphs.errors[0]}[int(status[0])]
        raise RuntimeError("alignment failed: %s" % why)

    def align_batch(self, loglikes, lengths, texts, beam=None):
        """loglikes [N, Tmax, P] (device, prior subtracted), lengths[N], texts[N]: one compile call and one launch on the
        current stream.  Returns a list of align() results, None where an utterance failed."""
        self._graph_model()
        x = self._as_device(loglikes, 3)
        lengths = [int(t) for t in lengths]
        _, ali, costs, status = self._viterbi(x, lengths, texts, self.beam if beam is None else beam)
        return [self._result(ali[n], costs[n], lengths[n]) if status[n] == ALIGN_OK else None for n in range(len(lengths))]


class GraphSupervision:
    """Alignment-free ("flat-start" / e2e) chain supervision of a MINIBATCH: the training graphs of its transcripts
    (AlignmentGraphs), over which the numerator sums every path of exactly frames_per_sequence[n] frames
    (csrc/chain_num_graph.hip).  status[n]: 0 compiled, 2 no path of that many frames -- the utterance then takes no part
    in the objective (outputs and gradient rows 0) -- and errors[n] says why."""

    def __init__(self, graphs, weight=1.0, label_dim=None):
        self.graphs = graphs
        self.weight = float(weight)
        self.label_dim = label_dim
        self.num_sequences = graphs.n
        self.frames_per_sequence = [int(t) for t in graphs.frames]
        self.status = list(graphs.status)
        self.errors = list(graphs.errors)

    def __len__(self):
        return self.num_sequences


def graph_supervisions(aligner, texts, frames, transition_scale=0.0, self_loop_scale=0.0, weight=1.0):
    """GraphSupervision of a minibatch of transcripts in one compile call.  aligner: a MappedAligner with tree and lexicon
    (from_files / from_models); frames[n]: network-rate frames of utterance n.  With both scales 0 (the default) only the
    lexicon's costs remain in the graph, like the unweighted alignment-based supervisions.  Raises when a transcript does
    not compile (status 3: a word outside the lexicon, a phone without a model)."""
    model, lexicon = aligner._graph_model_scaled(transition_scale, self_loop_scale)
    graphs = AlignmentGraphs(model, lexicon, [aligner._words(t) for t in texts], frames)
    for n, st in enumerate(graphs.status):
        if st == ALIGN_ERROR:
            raise _lib.Pk2Error("graph_supervisions: utterance %d: %s" % (n, graphs.errors[n]))
    return GraphSupervision(graphs, weight, aligner.transition_model.num_pdfs())


def _as_graph_supervision(supervisions):
    """The GraphSupervision behind the `supervisions` argument of the chain entry points, or None for Supervision lists."""
    if isinstance(supervisions, GraphSupervision):
        return supervisions
    if isinstance(supervisions, (list, tuple)):
        kinds = [isinstance(s, GraphSupervision) for s in supervisions]
        if any(kinds):
            if not all(kinds):
                raise TypeError("a list of supervisions mixes GraphSupervision and Supervision")
            if len(supervisions) != 1:
                raise TypeError("a GraphSupervision holds the whole minibatch: pass one, not a list of %d" % len(supervisions))
            return supervisions[0]
    return None


class _SupervisionBatch:
    """Concatenates per-utterance supervisions and ships them to the device in one
    pinned H2D copy (a few tens of KB)."""

    def __init__(self, sups, device):
        n = len(sups)
        arcs = np.cumsum([0] + [s.src.shape[0] for s in sups])
        self.total_arcs = int(arcs[-1])
        self.state_off = np.cumsum([0] + [s.num_states for s in sups]).astype(np.int32)
        self.final_off = np.cumsum([0] + [s.final_states.shape[0] for s in sups]).astype(np.int32)
        self.lengths = np.asarray([s.frames_per_sequence for s in sups], dtype=np.int32)
        frame_off = np.concatenate([s.frame_offsets + arcs[i] for i, s in enumerate(sups)]).astype(np.int32)
        ints = [np.concatenate([s.src for s in sups]), np.concatenate([s.dst for s in sups]),
                np.concatenate([s.pdf for s in sups]), frame_off,
                np.concatenate([s.final_states for s in sups])]
        flts = [np.concatenate([s.arc_weight for s in sups]), np.concatenate([s.final_weights for s in sups])]
        sizes = [a.shape[0] for a in ints + flts]
        offs = np.cumsum([0] + [(-(-s // 64)) * 64 for s in sizes])
        host = torch.empty(int(offs[-1]), dtype=torch.int32).pin_memory()
        hv = host.numpy()
        for a, o in zip(ints, offs[:5]):
            hv[o:o + a.shape[0]] = a
        for a, o in zip(flts, offs[5:7]):
            hv[o:o + a.shape[0]] = a.view(np.int32)
        self._host = host
        self.dev = host.to(device, non_blocking=True)
        base = self.dev.data_ptr()
        p = [C.c_void_p(base + int(o) * 4) for o in offs[:7]]
        self.struct = _lib.NumBatch(p[0], p[1], p[2], p[5], p[3], _lib.ptr(self.state_off), p[4], p[6],
                                    _lib.ptr(self.final_off), self.total_arcs, int(np.diff(arcs).max()) if n else 0)
        self.n = n


_workspace_cache = {}


def _workspace(device, nbytes):
    key = (device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspace_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _workspace_cache[key] = None
        ws = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _workspace_cache[key] = ws
    return ws


def compute_chain_objf_and_deriv(opts, den_graph, supervisions, nnet_output, lengths=None, operator_form=False):
    """Batched kaldi.chain.compute_chain_objf_and_deriv (reference ops/ops.py:265-267).

    nnet_output: f32 CUDA tensor [N, T, P] (or [T, P] with a single Supervision); row t of
    sequence n is frame t.  Returns (out, grad): out is a device tensor [3, N] =
    (objf, log p_num, log p_den) per sequence, grad is d objf / d nnet_output with
    xent_regularize * numerator posterior already added (zeros on padding frames).
    operator_form=True (ops.ChainObjtiveBatch): out is [3 N + 1] -- the same three rows followed by sum_n objf[n] -- and grad
    holds MINUS the derivative, what the reference operator's backward returns (ops/ops.py:276-280); both come out of the
    library call itself, no torch kernel runs around it.
    """
    gs = _as_graph_supervision(supervisions)
    _lib.require_gpu()
    if gs is not None:
        return _graph_objf_and_deriv(opts, den_graph, gs, nnet_output, operator_form)
    if isinstance(supervisions, Supervision):
        supervisions = [supervisions]
    x = nnet_output
    if x.dim() == 2:
        x = x.unsqueeze(0)
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1
    N, T, P = x.shape
    assert N == len(supervisions) and P == den_graph.num_pdfs()
    sb = _SupervisionBatch(supervisions, x.device)
    assert int(sb.lengths.max()) <= T
    weight = supervisions[0].weight
    L = _lib.lib()
    Tmax = int(sb.lengths.max())
    bound = max(sb.total_arcs, int(sb.lengths.sum()) + N)
    nbytes = L.pk2_chain_workspace_bytes(den_graph._h, N, Tmax, bound)
    ws = _workspace(x.device, nbytes)
    grad = torch.empty_like(x)
    if Tmax < T:
        grad[:, Tmax:].zero_()
    if operator_form:
        out = torch.empty(3 * N + 1, dtype=torch.float32, device=x.device)
        _lib.check(L.pk2_chain_objf_and_deriv_op(den_graph._h, _lib.ptr(x), x.stride(0), x.stride(1),
                                                 _lib.ptr(sb.lengths), N, C.byref(sb.struct),
                                                 float(opts.leaky_hmm_coefficient), float(opts.xent_regularize),
                                                 float(opts.l2_regularize), float(weight), _lib.ptr(grad),
                                                 grad.stride(0), grad.stride(1), _lib.ptr(out), _lib.ptr(ws),
                                                 ws.numel(), -1.0, _lib.ptr(out[3 * N:]), _lib.stream_ptr(x.device)))
        out._pk2_keepalive = sb
        return out, grad
    out = torch.empty(3, N, dtype=torch.float32, device=x.device)
    _lib.check(L.pk2_chain_objf_and_deriv(den_graph._h, _lib.ptr(x), x.stride(0), x.stride(1),
                                          _lib.ptr(sb.lengths), N, C.byref(sb.struct),
                                          float(opts.leaky_hmm_coefficient), float(opts.xent_regularize),
                                          float(opts.l2_regularize), float(weight), _lib.ptr(grad),
                                          grad.stride(0), grad.stride(1), _lib.ptr(out), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr(x.device)))
    # keep the pinned staging buffer alive until the stream has consumed it
    out._pk2_keepalive = sb
    return out, grad


NUM_CARRIERS = ("none", "stand_alone", "occupancy_lds_row", "occupancy_gather", "persistent", "side_stream")


def last_num_route():
    """Where the supervised numerator's forward-backward ran in the last compute_chain_objf_and_deriv call of the process
    (csrc/chain_internal.h: NumRoute), as a dict: staged (frame table and arcs copied into LDS), carrier (one of
    NUM_CARRIERS), threads (of the routine: 256, 128 = the two-wave one, 64) and lds_bytes.  Reporting only."""
    out = np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib().pk2_chain_debug_num_route(_lib.ptr(out)))
    return dict(staged=bool(out[0]), carrier=NUM_CARRIERS[int(out[1])], threads=int(out[2]), lds_bytes=int(out[3]))


def _graph_objf_and_deriv(opts, den_graph, gs, nnet_output, operator_form):
    """compute_chain_objf_and_deriv for a GraphSupervision: one library call, no torch kernel around it."""
    x = nnet_output
    if x.dim() == 2:
        x = x.unsqueeze(0)
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1
    N, T, P = x.shape
    graphs = gs.graphs
    Tmax = int(graphs.frames.max())
    assert N == graphs.n and P == den_graph.num_pdfs() and Tmax <= T
    L = _lib.lib()
    dev = graphs.to_device(x.device)
    ws = _workspace(x.device, L.pk2_chain_graph_workspace_bytes(den_graph._h, graphs._h))
    grad = torch.empty_like(x)
    if Tmax < T:
        grad[:, Tmax:].zero_()
    opt = (float(opts.leaky_hmm_coefficient), float(opts.xent_regularize), float(opts.l2_regularize), float(gs.weight))
    if operator_form:
        out = torch.empty(3 * N + 1, dtype=torch.float32, device=x.device)
        _lib.check(L.pk2_chain_objf_and_deriv_graph_op(den_graph._h, _lib.ptr(x), x.stride(0), x.stride(1), graphs._h, _lib.ptr(dev),
                                                       *opt, _lib.ptr(grad), grad.stride(0), grad.stride(1), _lib.ptr(out),
                                                       _lib.ptr(ws), ws.numel(), -1.0, _lib.ptr(out[3 * N:]),
                                                       _lib.stream_ptr(x.device)))
    else:
        out = torch.empty(3, N, dtype=torch.float32, device=x.device)
        _lib.check(L.pk2_chain_objf_and_deriv_graph(den_graph._h, _lib.ptr(x), x.stride(0), x.stride(1), graphs._h, _lib.ptr(dev),
                                                    *opt, _lib.ptr(grad), grad.stride(0), grad.stride(1), _lib.ptr(out),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    out._pk2_keepalive = (gs, dev)
    return out, grad


def num_graph_forward_backward(graphs, nnet_output, scale=1.0, grad=None):
    """Alignment-free numerator only: (log p_num [N], posteriors [N, T, P]); the first carries the device statuses as
    `.status`.  graphs: AlignmentGraphs or GraphSupervision.  Test / profiling hook, the twin of den_forward_backward; with
    `grad` given, scale * posterior is added into it (rows of utterances without a graph and rows past an utterance's frames
    are not touched)."""
    _lib.require_gpu()
    graphs = getattr(graphs, "graphs", graphs)
    x = nnet_output
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1
    N, T, P = x.shape
    assert N == graphs.n and int(graphs.frames.max()) <= T
    L = _lib.lib()
    dev = graphs.to_device(x.device)
    ws = _workspace(x.device, L.pk2_num_graph_workspace_bytes(graphs._h))
    if grad is None:
        grad = torch.zeros(N, T, P, dtype=torch.float32, device=x.device)
    assert grad.is_cuda and grad.dtype == torch.float32 and grad.shape == x.shape and grad.stride(2) == 1
    lp = torch.empty(N, dtype=torch.float32, device=x.device)
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    _lib.check(L.pk2_num_graph_fwd_bwd(graphs._h, _lib.ptr(dev), _lib.ptr(x), x.stride(0), x.stride(1), P, T, float(scale),
                                       _lib.ptr(grad), grad.stride(0), grad.stride(1), _lib.ptr(lp), _lib.ptr(status),
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    lp._pk2_keepalive = (graphs, dev)
    lp.status = status
    return lp, grad


def den_forward_backward(den_graph, nnet_output, lengths, leaky):
    """Denominator only: (log p_den [N], occupancies [N,T,P]).  Test / profiling hook."""
    _lib.require_gpu()
    x = nnet_output
    N, T, P = x.shape
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    L = _lib.lib()
    Tmax = int(lengths.max())
    nbytes = L.pk2_chain_workspace_bytes(den_graph._h, N, Tmax, 0)
    ws = _workspace(x.device, nbytes)
    gamma = torch.zeros_like(x)
    lp = torch.empty(N, dtype=torch.float32, device=x.device)
    _lib.check(L.pk2_chain_den_fwd_bwd(den_graph._h, _lib.ptr(x), x.stride(0), x.stride(1),
                                       _lib.ptr(lengths), N, float(leaky), _lib.ptr(lp), _lib.ptr(gamma),
                                       gamma.stride(0), gamma.stride(1), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr(x.device)))
    return lp, gamma
