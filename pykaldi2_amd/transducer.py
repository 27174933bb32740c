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

The pruned second stage (csrc/transducer_pruned.hip), for a nonlinear joiner that is evaluated on a band of S
predictor rows per frame only:

    loss, grad_am, grad_lm, status, begin, gamma = transducer.loss_grad_and_ranges(am, lm, lengths, labels, S)
    h = transducer.join_pruned(enc, pred, begin, lengths, label_counts, S)        # [N, T, S, J]; ops.PrunedJoin under autograd
    loss, grad, status = transducer.pruned_loss_and_grad(logits, begin, lengths, labels)     # logits [N, T, S, V]

ops.PrunedTransducerLoss is the autograd form of the last.  Its logits have no restriction on their numeric range.

Beam search for either head (csrc/transducer_beam.hip), one launch for all frames:

    nbest = transducer.beam_search(am, lengths, table, nbest=4, blank=0, beam=8)                       # the additive head
    nbest = transducer.beam_search(enc, lengths, pred, joiner=(w_out, b_out), blank=0, beam=8)       # through the joiner
"""
import numpy as np
import torch

from . import _beam, _lib
from .chain import _workspace

TRANSDUCER_OK, TRANSDUCER_NUMERIC = 0, 3      # PK2_TRANSDUCER_OK / PK2_TRANSDUCER_NUMERIC
TRANSDUCER_RANGES = 2                         # PK2_TRANSDUCER_RANGES (the pruned loss only): begin is not a valid band
MAX_LABELS = 1023                             # PK2_TRANSDUCER_MAX_LABELS
MAX_PRUNE_RANGE = 32                          # PK2_TRANSDUCER_MAX_PRUNE_RANGE
PRUNED_SHORT_ROWS = 256                       # PK2_TRANSDUCER_PRUNED_SHORT_ROWS: below it 16 lanes serve a row, else a wave
MAX_BEAM, MAX_BEAM_TOKENS = 32, 32            # PK2_TRANSDUCER_BEAM_MAX / PK2_TRANSDUCER_BEAM_MAX_TOKENS
MAX_BEAM_JOIN, MAX_BEAM_SYMBOLS = 512, 31     # PK2_TRANSDUCER_BEAM_MAX_JOIN / PK2_TRANSDUCER_BEAM_MAX_SYMBOLS


def _check_range(S):
    if isinstance(S, bool) or int(S) != S or not 2 <= S <= MAX_PRUNE_RANGE:
        raise ValueError("transducer: prune range %r outside [2, %d]" % (S, MAX_PRUNE_RANGE))
    return int(S)


def pack(lengths, labels, num_frames, num_rows, num_classes, blank=0, weights=None, prune_range=None):
    """The packed descriptor of include/pk2hip.h (pk2_transducer_loss_and_grad) as an int32 array, after checking the
    arguments: ValueError for a label that is the blank or outside [0, num_classes), more than MAX_LABELS labels or more
    than num_rows - 1 (the predictor tensor's rows), a length outside [1, num_frames]; with prune_range = S, also for an
    utterance that a band of S rows moving at most S - 1 a frame cannot cover: max(0, U + 1 - S) > (S - 1)(T - 1)."""
    if prune_range is not None:
        prune_range = _check_range(prune_range)
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
        if prune_range is not None and max(0, U + 1 - prune_range) > (prune_range - 1) * (T - 1):
            raise ValueError("transducer: utterance %d: %d labels cannot be covered by a band of %d rows over %d frames"
                             % (n, U, prune_range, T))
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


def _first_stage(am, lm, lengths, labels, blank, weights, time_major, prune_range=None):
    """transducer_loss_and_grad's call; returns its four results and (host, dev, ws, N, T) for a follow-on on the same stream."""
    a = _logits(am, "am").transpose(0, 1) if time_major else _logits(am, "am")
    p = _logits(lm, "lm")
    N, T, V = a.shape
    if p.shape[0] != N or p.shape[2] != V or p.device != a.device:
        raise ValueError("transducer: lm %s does not go with am %s" % (tuple(lm.shape), tuple(am.shape)))
    host = pack(lengths, labels, T, p.shape[1], V, blank, weights, prune_range)
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
    return (loss, g, gl, status), (host, dev, ws, N, T)


def transducer_loss_and_grad(am, lm, lengths, labels, blank=0, weights=None, time_major=False):
    """Transducer loss and its gradients with respect to both logit tensors, in one library call.

    am: float32 device tensor [N, T, V] ([T, N, V] with time_major), lm: [N, U + 1, V] with U + 1 > every label count; unit
    column stride, any row and utterance strides (served in place); rows past an utterance's frames / labels + 1 are not
    read.  lengths: N frame counts >= 1.  labels: N int sequences (0 <= U <= 1023, none the blank).  weights: per-utterance
    float32 factors w_n of the gradients (default 1).
    Returns (loss float64 [N] = -log p(labels | am, lm), grad_am and grad_lm float32 shaped and ordered like their inputs
    with the rows past the lengths 0, status int32 [N]): status 3 = outside the supported range (module docstring), loss 0
    and gradients 0 for that utterance, the others bit-identical."""
    return _first_stage(am, lm, lengths, labels, blank, weights, time_major)[0]


def loss_grad_and_ranges(am, lm, lengths, labels, S, blank=0, weights=None, time_major=False):
    """transducer_loss_and_grad and, from the occupancies it computed anyway, the pruning ranges of the second stage: the
    normaliser and the lattice run once, one more launch reads the workspace they left on the stream.

    Returns (loss, grad_am, grad_lm, status, begin, gamma): the first four exactly transducer_loss_and_grad's; gamma float32
    [N, T, Umax + 1] = occ_x + occ_y (Umax the largest label count; zeros past T_n / U_n and for a status-3 utterance); begin
    int32 [N, T]: frame t of utterance n sees the predictor rows u = begin[t] + s, s = 0..S-1.  With Bmax = max(0, U + 1 - S),
    every scan backwards over t:
        win[t,s] = sum_{u=s}^{min(s+S-1,U)} gamma[t,u]       in float64, ascending u, every window on its own
        raw[t]   = argmax_{0<=s<=Bmax} win[t,s], ties to the lowest s, clamped into [max(0, Bmax-(S-1)(T-1-t)), min(Bmax, (S-1)t)]
        b[t]     = min_{t'>=t} raw[t']       begin[t] = max_{t'>=t} (b[t'] - (S-1)(t'-t))       begin[t] = 0 for t >= T_n
    so begin[0] = 0, begin[T-1] = Bmax and 0 <= begin[t+1] - begin[t] <= S-1.  2 <= S <= 32; ValueError for an utterance
    with Bmax > (S-1)(T-1), which no such band covers."""
    S = _check_range(S)
    out, (host, dev, ws, N, T) = _first_stage(am, lm, lengths, labels, blank, weights, time_major, S)
    U1 = max(len(seq) for seq in labels) + 1
    device = out[0].device
    begin = torch.empty((N, T), dtype=torch.int32, device=device)
    gamma = torch.empty((N, T, U1), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().pk2_transducer_ranges(_lib.ptr(host), _lib.ptr(dev), host.numel(), N, S, T, U1, _lib.ptr(out[3]), _lib.ptr(ws),
                                                ws.numel(), _lib.ptr(begin), _lib.ptr(gamma), _lib.stream_ptr(device)))
    return out + (begin, gamma)


def _begin(begin, N, T, device):
    if begin.dtype != torch.int32 or tuple(begin.shape) != (N, T) or begin.device != device:
        raise ValueError("transducer: begin must be int32 [%d, %d] on the logits' device" % (N, T))
    return begin.contiguous()


def pruned_loss_and_grad(logits, begin, lengths, labels, blank=0, weights=None):
    """The transducer loss and its gradient on the 4-D logits of a joiner that was evaluated on a band, in one library call
    of three launches.

    logits: float32 device tensor [N, T, S, V], unnormalised, any numeric range; unit column stride, any other strides (served
    in place).  Row (t, s) is the joiner's output for frame t and predictor row u = begin[t] + s.  begin: int32 [N, T] on the
    device, from loss_grad_and_ranges or from anywhere: the device validates it before using it.  lengths, labels, weights:
    as for transducer_loss_and_grad.
    Returns (loss float64 [N], grad float32 [N, T, S, V] with zeros in the rows t >= T_n and u > U_n, status int32 [N]):
    status 2 (TRANSDUCER_RANGES) = begin[0] != 0, a step outside [0, S-1], begin[T-1] + S - 1 < U or a negative entry;
    status 3 = a row's maximum or the total is not finite; either way loss 0 and gradient 0, the others bit-identical."""
    if logits.dim() != 4 or logits.dtype != torch.float32 or logits.stride(3) != 1:
        raise ValueError("transducer: logits must be float32 [N, T, S, V] with a unit column stride")
    z = logits.detach()
    N, T, S, V = z.shape
    S = _check_range(S)
    bg = _begin(begin, N, T, z.device)
    host = pack(lengths, labels, T, MAX_LABELS + 1, V, blank, weights)
    if len(labels) != N:
        raise ValueError("transducer: %d label sequences for %d utterances" % (len(labels), N))
    _lib.require_gpu()
    L = _lib.lib()
    host = torch.from_numpy(host).pin_memory()
    dev = host.to(z.device, non_blocking=True)
    ws = _workspace(z.device, L.pk2_transducer_pruned_workspace_bytes(N, T, S, V))
    grad = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    loss = torch.empty(N, dtype=torch.float64, device=z.device)
    status = torch.empty(N, dtype=torch.int32, device=z.device)
    _lib.check(L.pk2_transducer_pruned_loss_and_grad(_lib.ptr(host), _lib.ptr(dev), host.numel(), N, _lib.ptr(z), z.stride(0), z.stride(1),
                                                     z.stride(2), T, S, V, int(blank), _lib.ptr(bg), _lib.ptr(grad), _lib.ptr(loss),
                                                     _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(z.device)))
    loss._pk2_keepalive = (host, dev, bg)
    return loss, grad, status


def _join_args(enc, pred, begin, lengths, label_counts):
    for x, name in ((enc, "enc"), (pred, "pred")):
        if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
            raise ValueError("transducer: %s must be float32 [N, rows, J] with a unit column stride" % name)
    N, T, J = enc.shape
    if pred.shape[0] != N or pred.shape[2] != J or pred.device != enc.device:
        raise ValueError("transducer: pred %s does not go with enc %s" % (tuple(pred.shape), tuple(enc.shape)))
    lens = np.stack([np.asarray(lengths, dtype=np.int64).reshape(-1), np.asarray(label_counts, dtype=np.int64).reshape(-1)], 1)
    if lens.shape[0] != N or lens.min() < 0 or lens[:, 0].max() > T or lens[:, 1].max() >= pred.shape[1]:
        raise ValueError("transducer: lengths and label counts do not fit enc %s and pred %s" % (tuple(enc.shape), tuple(pred.shape)))
    host = torch.from_numpy(lens.astype(np.int32)).pin_memory()
    return host, host.to(enc.device, non_blocking=True), _begin(begin, N, T, enc.device)


def join_pruned(enc, pred, begin, lengths, label_counts, S, tanh=True):
    """The banded join for a joiner network, one launch: h[n, t, s, :] = tanh(enc[n, t, :] + pred[n, begin[t] + s, :]) (the
    plain sum with tanh=False) as float32 [N, T, S, J]; zeros for t >= lengths[n] and for begin[t] + s outside
    [0, label_counts[n]].  enc [N, T, J], pred [N, U + 1, J]: float32, unit column stride.  The two gathered [N, T, S, J]
    copies are never made.  ops.PrunedJoin is the autograd form."""
    S = _check_range(S)
    host, dev, bg = _join_args(enc, pred, begin, lengths, label_counts)
    e, p = enc.detach(), pred.detach()
    N, T, J = e.shape
    _lib.require_gpu()
    h = torch.empty((N, T, S, J), dtype=torch.float32, device=e.device)
    _lib.check(_lib.lib().pk2_transducer_join(_lib.ptr(host), _lib.ptr(dev), N, _lib.ptr(e), e.stride(0), e.stride(1), _lib.ptr(p),
                                              p.stride(0), p.stride(1), _lib.ptr(bg), T, p.shape[1], S, J, int(bool(tanh)), _lib.ptr(h),
                                              _lib.stream_ptr(e.device)))
    h._pk2_keepalive = (host, dev, bg)
    return h


def join_pruned_backward(dh, h, begin, lengths, label_counts, num_rows, tanh=True):
    """(d_enc [N, T, J], d_pred [N, num_rows, J]) of join_pruned from dh and its output h [N, T, S, J], one launch, no
    atomics: d_enc[t] sums its S band rows in ascending s, d_pred[u] the frames whose band holds u in ascending t."""
    N, T, S, J = h.shape
    dh = dh.detach().to(torch.float32).contiguous()
    lens = np.stack([np.asarray(lengths, dtype=np.int64).reshape(-1), np.asarray(label_counts, dtype=np.int64).reshape(-1)], 1)
    if tuple(dh.shape) != tuple(h.shape) or not h.is_contiguous() or lens.shape[0] != N:
        raise ValueError("transducer: dh %s does not go with h %s" % (tuple(dh.shape), tuple(h.shape)))
    host = torch.from_numpy(lens.astype(np.int32)).pin_memory()
    dev = host.to(h.device, non_blocking=True)
    bg = _begin(begin, N, T, h.device)
    d_enc = torch.empty((N, T, J), dtype=torch.float32, device=h.device)
    d_pred = torch.empty((N, int(num_rows), J), dtype=torch.float32, device=h.device)
    _lib.check(_lib.lib().pk2_transducer_join_backward(_lib.ptr(host), _lib.ptr(dev), N, _lib.ptr(dh), _lib.ptr(h), _lib.ptr(bg), T,
                                                       int(num_rows), S, J, int(bool(tanh)), _lib.ptr(d_enc), _lib.ptr(d_pred),
                                                       _lib.stream_ptr(h.device)))
    d_enc._pk2_keepalive = (host, dev, bg, dh)
    return d_enc, d_pred


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


def beam_search_raw(am_or_enc, lengths, table_or_pred, blank=0, beam=4, top_tokens=8, max_symbols=2, joiner=None, time_major=False):
    """Transducer beam search with a stateless predictor of context 1 on the device (csrc/transducer_beam.hip):
    one launch, nothing read back.  Time-synchronous; per frame at most max_symbols (1..31) rounds in which every hypothesis
    moves on with the blank and is extended by the top_tokens (1..32, clamped to V - 1) non-blank columns of its largest
    logit, the `beam` (1..32) most probable extensions going into the next round; at the frame's end the blank moves, merged
    by prefix, are cut to the `beam` most probable.  Scores are float64 log-probabilities, the log-softmax float32.

    additive head (joiner=None): am float32 [N, T, V] ([T, N, V] with time_major) and table [V, V], greedy_decode's operands:
    z(t, prev) = am[t] + table[prev].  joiner=(w_out [V, J], b_out [V]): enc [N, T, J] (the joiner's enc layer applied to the
    encoder output) and pred [V, J] (its pred layer applied to the table rows): z(t, prev) = tanh(enc[t] + pred[prev]) w_out^T
    + b_out, J <= 512.  Unit column stride, any other strides (served in place); rows past a length are never read.
    Returns device tensors (tokens int32 [N, beam, T * max_symbols] left-aligned with -1 behind, lens int32 [N, beam] with -1
    for unused slots, scores float64 [N, beam] non-increasing with -inf for unused slots, status int32 [N]): status 3
    (TRANSDUCER_NUMERIC) = a row's maximum or normaliser was not finite, all slots unused; the others are unaffected.  An
    utterance of 0 frames returns the empty prefix with score 0."""
    x = am_or_enc
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("transducer: %s must be float32 [N, T, %s] with a unit column stride" % (("enc", "J") if joiner else ("am", "V")))
    x = x.detach().transpose(0, 1) if time_major else x.detach()
    N, T, D = x.shape
    rows = table_or_pred
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.stride(1) != 1 or rows.device != x.device or rows.shape[1] != D:
        raise ValueError("transducer: %s must be float32 [V, %d] with a unit column stride, on the first operand's device"
                         % ("pred" if joiner else "the table", D))
    V = rows.shape[0]
    w = b = None
    if joiner is None:
        if V != D:
            raise ValueError("transducer: the table must be [%d, %d], not %s" % (D, D, tuple(rows.shape)))
    else:
        w, b = joiner
        if D > MAX_BEAM_JOIN:
            raise ValueError("transducer: joiner width %d beyond %d" % (D, MAX_BEAM_JOIN))
        if (w.dim() != 2 or tuple(w.shape) != (V, D) or w.dtype != torch.float32 or w.stride(1) != 1 or w.device != x.device or
                b.dim() != 1 or b.shape[0] != V or b.dtype != torch.float32 or b.device != x.device):
            raise ValueError("transducer: w_out %s / b_out %s do not go with enc %s and pred %s"
                             % (tuple(w.shape), tuple(b.shape), tuple(am_or_enc.shape), tuple(rows.shape)))
        w, b = w.detach(), b.detach().contiguous()
    beam = _beam.limit(beam, MAX_BEAM, "beam", "transducer")
    top_tokens = _beam.limit(top_tokens, MAX_BEAM_TOKENS, "top_tokens", "transducer")
    max_symbols = _beam.limit(max_symbols, MAX_BEAM_SYMBOLS, "max_symbols", "transducer")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if N < 1 or lengths.shape[0] != N or lengths.min() < 0 or lengths.max() > T:
        raise ValueError("transducer: %d lengths for %d utterances of at most %d frames" % (lengths.shape[0], N, T))
    if V < 2 or not 0 <= blank < V:
        raise ValueError("transducer: blank %d of %d columns" % (blank, V))
    _lib.require_gpu()
    L = _lib.lib()
    host = torch.from_numpy(lengths.astype(np.int32)).pin_memory()
    dev = host.to(x.device, non_blocking=True)
    rows = rows.detach()
    J = 0 if joiner is None else D
    ws = _workspace(x.device, L.pk2_transducer_beam_workspace_bytes(N, T, V, beam, max_symbols, J))
    tokens = torch.empty((N, beam, T * max_symbols), dtype=torch.int32, device=x.device)
    lens = torch.empty((N, beam), dtype=torch.int32, device=x.device)
    scores = torch.empty((N, beam), dtype=torch.float64, device=x.device)
    status = torch.empty(N, dtype=torch.int32, device=x.device)
    _lib.check(L.pk2_transducer_beam_search(_lib.ptr(host), _lib.ptr(dev), N, _lib.ptr(x), x.stride(0), x.stride(1), T, _lib.ptr(rows),
                                            rows.stride(0), _lib.ptr(w), w.stride(0) if J else 0, _lib.ptr(b), J, V, int(blank), beam,
                                            top_tokens, max_symbols, _lib.ptr(tokens), _lib.ptr(lens), _lib.ptr(scores), _lib.ptr(status),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    scores._pk2_keepalive = (host, dev, b)      # until the stream has consumed them
    return tokens, lens, scores, status


def beam_search(am_or_enc, lengths, table_or_pred, nbest=1, **kw):
    """beam_search_raw and ONE copy to the host: per utterance a list of at most nbest (token list, score), best first."""
    tokens, lens, scores, _ = beam_search_raw(am_or_enc, lengths, table_or_pred, **kw)
    return _beam.nbest_lists(tokens, lens, scores, nbest)
