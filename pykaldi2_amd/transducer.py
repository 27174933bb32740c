"""Transducer (RNN-T) loss with an additive joint on the device (csrc/transducer.hip).

    loss, grad_am, grad_lm, status = transducer.transducer_loss_and_grad(am, lm, lengths, labels, blank=0)
    hyps = transducer.greedy_decode(am, lengths, table, blank=0)

ops.TransducerLoss is the autograd form.  am [N, T, V] are the encoder's UNNORMALISED logits and lm [N, U + 1, V] the
predictor's (row u: after u labels); the joint is their sum, z[t, u, .] = am[t, .] + lm[u, .], and neither the [T, U + 1, V]
tensor of it nor its gradient is ever stored: the normaliser and both gradients are matrix products over exponentials, the
lattice a wavefront over the T x (U + 1) grid.  One library call of seven launches, bit-reproducible.

Supported range: float32 logits whose row spread (max - min over the columns) of am PLUS that of lm is at most 60, so that the
factorised normaliser sum_v exp(am - max am) exp(lm - max lm) >= e^-60 is a normal float32 with room for the posteriors
divided by it.  Beyond that range an utterance may come back with status 3 (TRANSDUCER_NUMERIC): loss 0 and gradient rows 0,
nothing aborts.  At most MAX_LABELS labels per utterance.
"""
import numpy as np
import torch

from . import _lib
from .chain import _workspace

TRANSDUCER_OK, TRANSDUCER_NUMERIC = 0, 3      # PK2_TRANSDUCER_OK / PK2_TRANSDUCER_NUMERIC
MAX_LABELS = 1023                             # PK2_TRANSDUCER_MAX_LABELS


def pack(lengths, labels, num_frames, num_rows, num_classes, blank=0, weights=None):
    """The packed descriptor of include/pk2hip.h (pk2_transducer_loss_and_grad) as an int32 array, after checking the
    arguments: ValueError for a label that is the blank or outside [0, num_classes), more than MAX_LABELS labels or more
    than num_rows - 1 (the predictor tensor's rows), a length outside [1, num_frames]."""
    N = len(labels)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if N < 1 or lengths.shape[0] != N:
        raise ValueError("transducer: %d label sequences for %d lengths" % (N, lengths.shape[0]))
    if num_classes < 2 or not 0 <= blank < num_classes:
        raise ValueError("transducer: blank %d of %d columns" % (blank, num_classes))
    w = np.ones(N, np.float32) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    if w.shape[0] != N:
        raise ValueError("transducer: %d weights for %d utterances" % (w.shape[0], N))
    head = np.zeros((N, 8), np.int32)
    parts, off = [], 8 * N
    for n, seq in enumerate(labels):
        lab = np.asarray(seq, dtype=np.int64).reshape(-1)
        T, U = int(lengths[n]), lab.shape[0]
        if U > MAX_LABELS:
            raise ValueError("transducer: utterance %d has %d labels (limit %d)" % (n, U, MAX_LABELS))
        if U + 1 > num_rows:
            raise ValueError("transducer: utterance %d needs %d predictor rows, the tensor has %d" % (n, U + 1, num_rows))
        if not 1 <= T <= num_frames:
            raise ValueError("transducer: utterance %d has length %d, the tensor %d frames" % (n, T, num_frames))
        if U and (lab.min() < 0 or lab.max() >= num_classes or (lab == blank).any()):
            raise ValueError("transducer: utterance %d: labels must be in [0, %d) and not the blank %d" % (n, num_classes, blank))
        order = np.argsort(lab, kind="stable")
        head[n, :5] = (T, U, TRANSDUCER_OK, off, off + U)
        parts += [lab, order, lab[order]]
        off += 3 * U
    head[:, 5] = w.view(np.int32)
    return np.concatenate([head.reshape(-1)] + parts).astype(np.int32)


def _logits(x, name):
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("transducer: %s must be float32 [N, rows, V] with a unit column stride" % name)
    return x.detach()


def transducer_loss_and_grad(am, lm, lengths, labels, blank=0, weights=None, time_major=False):
    """Transducer loss and its gradients with respect to both logit tensors, in one library call.

    am: float32 device tensor [N, T, V] ([T, N, V] with time_major), lm: [N, U + 1, V] with U + 1 > every label count; unit
    column stride, any row and utterance strides (served in place); rows past an utterance's frames / labels + 1 are not
    read.  lengths: N frame counts >= 1.  labels: N int sequences (0 <= U <= 1023, none the blank).  weights: per-utterance
    float32 factors w_n of the gradients (default 1).
    Returns (loss float64 [N] = -log p(labels | am, lm), grad_am and grad_lm float32 shaped and ordered like their inputs
    with the rows past the lengths 0, status int32 [N]): status 3 = outside the supported range (module docstring), loss 0
    and gradients 0 for that utterance, the others bit-identical."""
    a = _logits(am, "am").transpose(0, 1) if time_major else _logits(am, "am")
    p = _logits(lm, "lm")
    N, T, V = a.shape
    if p.shape[0] != N or p.shape[2] != V or p.device != a.device:
        raise ValueError("transducer: lm %s does not go with am %s" % (tuple(lm.shape), tuple(am.shape)))
    host = pack(lengths, labels, T, p.shape[1], V, blank, weights)
    if len(labels) != N:
        raise ValueError("transducer: %d label sequences for %d utterances" % (len(labels), N))
    _lib.require_gpu()
    L = _lib.lib()
    host = torch.from_numpy(host).pin_memory()
    dev = host.to(a.device, non_blocking=True)
    ws = _workspace(a.device, L.pk2_transducer_workspace_bytes(_lib.ptr(host), N, V))
    g = torch.empty(am.shape, dtype=torch.float32, device=a.device)      # dense, in the order of am's dimensions
    ga = g.transpose(0, 1) if time_major else g
    gl = torch.empty(p.shape, dtype=torch.float32, device=a.device)
    loss = torch.empty(N, dtype=torch.float64, device=a.device)
    status = torch.empty(N, dtype=torch.int32, device=a.device)
    _lib.check(L.pk2_transducer_loss_and_grad(_lib.ptr(host), _lib.ptr(dev), host.numel(), N, _lib.ptr(a), a.stride(0), a.stride(1), T,
                                              _lib.ptr(p), p.stride(0), p.stride(1), p.shape[1], V, int(blank), _lib.ptr(ga),
                                              ga.stride(0), ga.stride(1), _lib.ptr(gl), gl.stride(0), gl.stride(1), _lib.ptr(loss),
                                              _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(a.device)))
    loss._pk2_keepalive = (host, dev)      # the pinned block until the stream has consumed it
    return loss, g, gl, status


def greedy_decode_raw(am, lengths, table, blank=0, max_symbols=8, time_major=False):
    """Greedy decoding with a table predictor on the device, one launch: (tokens int32 [N, T * max_symbols] left-aligned
    with -1 behind, lens int32 [N]).  prev starts at the blank; per frame the argmax of am[t] + table[prev] (a float32 sum,
    ties to the lower column) is emitted and becomes prev until it is the blank or max_symbols were emitted."""
    a = _logits(am, "am").transpose(0, 1) if time_major else _logits(am, "am")
    N, T, V = a.shape
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.shape[0] != N or (N and (lengths.min() < 0 or lengths.max() > T)):
        raise ValueError("transducer: %d lengths for %d utterances of at most %d frames" % (lengths.shape[0], N, T))
    if table.dim() != 2 or table.dtype != torch.float32 or tuple(table.shape) != (V, V) or table.stride(1) != 1 or table.device != a.device:
        raise ValueError("transducer: the table must be float32 [%d, %d] with a unit column stride, on am's device" % (V, V))
    if N < 1 or not 0 <= blank < V or isinstance(max_symbols, bool) or int(max_symbols) != max_symbols or max_symbols < 1:
        raise ValueError("transducer: %d utterances, blank %d of %d columns, max_symbols %r" % (N, blank, V, max_symbols))
    _lib.require_gpu()
    host = torch.from_numpy(lengths.astype(np.int32)).pin_memory()
    dev = host.to(a.device, non_blocking=True)
    tokens = torch.empty((N, T * int(max_symbols)), dtype=torch.int32, device=a.device)
    lens = torch.empty(N, dtype=torch.int32, device=a.device)
    tab = table.detach()
    _lib.check(_lib.lib().pk2_transducer_greedy(_lib.ptr(host), _lib.ptr(dev), N, _lib.ptr(a), a.stride(0), a.stride(1), T, _lib.ptr(tab),
                                                tab.stride(0), V, int(blank), int(max_symbols), _lib.ptr(tokens), _lib.ptr(lens),
                                                _lib.stream_ptr(a.device)))
    lens._pk2_keepalive = (host, dev)
    return tokens, lens


def greedy_decode(am, lengths, table, blank=0, max_symbols=8, time_major=False):
    """greedy_decode_raw and ONE copy to the host: N int lists."""
    tokens, lens = greedy_decode_raw(am, lengths, table, blank, max_symbols, time_major)
    flat = torch.cat([tokens, lens[:, None]], dim=1).cpu().numpy()
    return [flat[n, :flat[n, -1]].tolist() for n in range(flat.shape[0])]
