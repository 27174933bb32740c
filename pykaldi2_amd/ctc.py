"""Connectionist temporal classification on the device (csrc/ctc.hip).

    loss, grad, status = ctc.ctc_loss_and_grad(logits, lengths, labels, blank=0)
    hyps = ctc.greedy_decode(logits, lengths, blank=0)
    nbest = ctc.beam_search(logits, lengths, nbest=4, beam=16, top_tokens=16, lm=phone_lm, lm_weight=0.5)

ops.CTCLoss is the autograd form.  The logits are UNNORMALISED network outputs (log-probabilities are the special case whose
rows have log-sum-exp 0): softmax, loss and gradient are one library call of three launches, bit-reproducible.

Supported range: float32 logits whose spread within a row (max - min over the columns) is at most 80, so that every
emission exp(x - logsumexp) is a normal float32; the recursions run in float64 and are rescaled every frame.  Beyond that
range an utterance may come back with status 3 (CTC_NUMERIC): loss 0 and gradient rows 0, nothing aborts.
"""
import numpy as np
import torch

from . import _beam, _lib
from .chain import _workspace

CTC_OK, CTC_NO_PATH, CTC_NUMERIC = 0, 2, 3      # PK2_CTC_OK / PK2_CTC_NO_PATH / PK2_CTC_NUMERIC
MAX_LABELS = 4095                               # PK2_CTC_MAX_LABELS
MAX_BEAM, MAX_TOP_TOKENS = 128, 32              # PK2_CTC_BEAM_MAX / PK2_CTC_BEAM_MAX_TOKENS


def pack(lengths, labels, num_frames, num_classes, blank=0, weights=None):
    """The packed descriptor of include/pk2hip.h (pk2_ctc_loss_and_grad) as an int32 array, after checking the arguments:
    ValueError for a label that is the blank or outside [0, num_classes), more than MAX_LABELS labels, a length outside
    [0, num_frames].  status (word 2 of an utterance): CTC_NO_PATH when there are fewer frames than labels + repeats."""
    N = len(labels)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if N < 1 or lengths.shape[0] != N:
        raise ValueError("ctc: %d label sequences for %d lengths" % (N, lengths.shape[0]))
    if num_classes < 2 or not 0 <= blank < num_classes:
        raise ValueError("ctc: blank %d of %d columns" % (blank, num_classes))
    w = np.ones(N, np.float32) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    if w.shape[0] != N:
        raise ValueError("ctc: %d weights for %d utterances" % (w.shape[0], N))
    head = np.zeros((N, 8), np.int32)
    parts, off = [], 8 * N
    for n, seq in enumerate(labels):
        lab = np.asarray(seq, dtype=np.int64).reshape(-1)
        T, L = int(lengths[n]), lab.shape[0]
        if L > MAX_LABELS:
            raise ValueError("ctc: utterance %d has %d labels (limit %d)" % (n, L, MAX_LABELS))
        if not 0 <= T <= num_frames:
            raise ValueError("ctc: utterance %d has length %d, the tensor %d frames" % (n, T, num_frames))
        if L and (lab.min() < 0 or lab.max() >= num_classes or (lab == blank).any()):
            raise ValueError("ctc: utterance %d: labels must be in [0, %d) and not the blank %d" % (n, num_classes, blank))
        order = np.argsort(lab, kind="stable")
        repeats = int((lab[1:] == lab[:-1]).sum())
        head[n, :5] = (T, L, CTC_OK if T >= max(1, L + repeats) else CTC_NO_PATH, off, off + L)
        parts += [lab, order, lab[order]]
        off += 3 * L
    head[:, 5] = w.view(np.int32)
    return np.concatenate([head.reshape(-1)] + parts).astype(np.int32)


def ctc_loss_and_grad(logits, lengths, labels, blank=0, weights=None, time_major=False):
    """CTC loss and its gradient with respect to the logits, in one library call.

    logits: float32 device tensor [N, T, P] ([T, N, P] with time_major), unit column stride, any row and utterance strides
    (served in place); rows past an utterance's length are not read.  lengths: N frame counts.  labels: N int sequences
    (0 <= L <= 4095, none the blank).  weights: per-utterance float32 factors w_n of the gradient (default 1).
    Returns (loss float64 [N] = -log p(labels | logits), grad float32 shaped and ordered like logits with rows past the
    length 0, status int32 [N]): status 2 = fewer frames than labels + repeats (no alignment), 3 = outside the supported
    range (module docstring); both give loss 0 and gradient 0 and leave the other utterances bit-identical."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1:
        raise ValueError("ctc: logits must be float32 [N, T, P] with a unit column stride")
    x = logits.detach().transpose(0, 1) if time_major else logits.detach()
    N, T, P = x.shape
    host = pack(lengths, labels, T, P, blank, weights)
    if len(labels) != N:
        raise ValueError("ctc: %d label sequences for %d utterances" % (len(labels), N))
    _lib.require_gpu()
    L = _lib.lib()
    host = torch.from_numpy(host).pin_memory()
    dev = host.to(x.device, non_blocking=True)
    ws = _workspace(x.device, L.pk2_ctc_workspace_bytes(_lib.ptr(host), N))
    g = torch.empty(logits.shape, dtype=torch.float32, device=x.device)      # dense, in the order of the logits' dimensions
    grad = g.transpose(0, 1) if time_major else g
    loss = torch.empty(N, dtype=torch.float64, device=x.device)
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    _lib.check(L.pk2_ctc_loss_and_grad(_lib.ptr(host), _lib.ptr(dev), host.numel(), N, _lib.ptr(x), x.stride(0), x.stride(1), T, P,
                                       int(blank), _lib.ptr(grad), grad.stride(0), grad.stride(1), _lib.ptr(loss), _lib.ptr(status),
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    loss._pk2_keepalive = (host, dev)      # the pinned block until the stream has consumed it
    return loss, g, status


def _beam_args(lengths, N, T, P, blank, beam, top_tokens, lm, lm_ids):
    """The host checks of beam_search_raw (ValueError before anything is launched): (lengths int32 [N], lm_ids int32 [P] or None)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.shape[0] != N or (N and (lengths.min() < 0 or lengths.max() > T)):
        raise ValueError("ctc: %d lengths for %d utterances of at most %d frames" % (lengths.shape[0], N, T))
    if N < 1 or P < 2 or not 0 <= blank < P:
        raise ValueError("ctc: %d utterances, blank %d of %d columns" % (N, blank, P))
    _beam.limit(beam, MAX_BEAM, "beam", "ctc")
    _beam.limit(top_tokens, MAX_TOP_TOKENS, "top_tokens", "ctc")
    if lm is None:
        if lm_ids is not None:
            raise ValueError("ctc: lm_ids without an LM")
        return lengths.astype(np.int32), None
    ids = np.arange(P, dtype=np.int64) if lm_ids is None else np.asarray(lm_ids, dtype=np.int64).reshape(-1)
    if ids.shape[0] != P:
        raise ValueError("ctc: lm_ids has %d entries for %d columns" % (ids.shape[0], P))
    unigrams = lm.word[int(lm.child_begin[0]):int(lm.child_begin[1])]
    missing = [c for c in np.flatnonzero(~np.isin(ids, unigrams)).tolist() if c != blank]
    if missing:
        raise ValueError("ctc: column %d (LM word id %d) has no unigram in the LM" % (missing[0], ids[missing[0]]))
    return lengths.astype(np.int32), (None if lm_ids is None else np.where(np.arange(P) == blank, 0, ids).astype(np.int32))


def beam_search_raw(logits, lengths, blank=0, beam=16, top_tokens=16, lm=None, lm_weight=1.0, insertion_bonus=0.0, lm_ids=None,
                    lm_eos=True, time_major=False):
    """CTC prefix beam search on the device (csrc/ctc_beam.hip), two launches, nothing read back.

    logits, lengths, time_major: as for ctc_loss_and_grad (served in place, rows past a length are not read).  Per frame a
    hypothesis stays or is extended by the top_tokens non-blank columns of the largest logit (clamped to P - 1); extensions
    that meet a hypothesis of the beam are merged into it; the `beam` (1..128) most probable survive.  lm: an ngram.NgramLM
    over the TOKENS (lm_ids: int [P], column -> LM word id, default the identity; every non-blank column needs a unigram):
    an extension by c is weighted exp(-lm_weight * cost(c | history) + insertion_bonus), and with lm_eos the final score
    gets -lm_weight * cost(</s> | history).
    Returns device tensors (tokens int32 [N, beam, T] left-aligned with -1 behind, lens int32 [N, beam] with -1 for unused
    slots, scores float64 [N, beam] = log(pb + pnb) (+ the </s> term), non-increasing, -inf for unused slots, status int32
    [N]): status 3 (CTC_NUMERIC) = a frame's best total was 0 or not finite, all slots unused; the others are unaffected."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1:
        raise ValueError("ctc: logits must be float32 [N, T, P] with a unit column stride")
    x = logits.detach().transpose(0, 1) if time_major else logits.detach()
    N, T, P = x.shape
    host, ids = _beam_args(lengths, N, T, P, blank, beam, top_tokens, lm, lm_ids)
    _lib.require_gpu()
    L = _lib.lib()
    host = torch.from_numpy(host).pin_memory()
    dev = host.to(x.device, non_blocking=True)
    ids_dev = None if ids is None else torch.from_numpy(ids).to(x.device)
    ws = _workspace(x.device, L.pk2_ctc_beam_workspace_bytes(N, T, P, int(beam), int(top_tokens)))
    tokens = torch.empty((N, int(beam), T), dtype=torch.int32, device=x.device)
    lens = torch.empty((N, int(beam)), dtype=torch.int32, device=x.device)
    scores = torch.empty((N, int(beam)), dtype=torch.float64, device=x.device)
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    _lib.check(L.pk2_ctc_beam_search(_lib.ptr(host), _lib.ptr(dev), N, _lib.ptr(x), x.stride(0), x.stride(1), T, P, int(blank), int(beam),
                                     int(top_tokens), lm.handle(x.device) if lm is not None else None, _lib.ptr(ids_dev),
                                     float(lm_weight), float(insertion_bonus), int(bool(lm_eos)), _lib.ptr(tokens), _lib.ptr(lens),
                                     _lib.ptr(scores), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    scores._pk2_keepalive = (host, dev, ids_dev, lm)      # until the stream has consumed them
    return tokens, lens, scores, status


def beam_search(logits, lengths, nbest=1, **kw):
    """beam_search_raw and ONE copy to the host: per utterance a list of at most nbest (token list, score), best first."""
    tokens, lens, scores, _ = beam_search_raw(logits, lengths, **kw)
    return _beam.nbest_lists(tokens, lens, scores, nbest)


def greedy_decode(logits, lengths, blank=0, time_major=False):
    """Best-path decoding: per-frame argmax, repeats collapsed, blanks dropped.  Returns N int lists.  torch ops on the device
    and one copy to the host: for the command line's error-rate printout, not a hot path."""
    x = logits.detach().transpose(0, 1) if time_major else logits.detach()
    best = x.argmax(dim=2)
    keep = torch.ones_like(best, dtype=torch.bool)
    keep[:, 1:] = best[:, 1:] != best[:, :-1]
    keep &= best != blank
    best, keep = best.cpu().numpy(), keep.cpu().numpy()
    return [best[n, :int(T)][keep[n, :int(T)]].tolist() for n, T in enumerate(lengths)]
