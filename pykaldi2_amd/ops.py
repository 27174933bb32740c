"""Loss operators with the reference's names and calling conventions (reference ops/ops.py).

  ChainObjtiveFunction.apply(loglikes, den_graph, supervision, chain_opts)   ops/ops.py:243-280
  ChainObjtiveBatch.apply(prediction, den_graph, supervisions, chain_opts)   the batched form
  CrossEntropy(logits, targets, ignore_index, reduction)                     nn.CrossEntropyLoss

Value / gradient convention kept from the reference: forward returns the
*objective* (log p_num - log p_den, to be maximised) and backward returns
minus its derivative regardless of ``grad_out`` (ops/ops.py:276-280), so
``loss.backward()`` followed by a descent step increases the objective.  Unlike
the reference, nothing is copied to the host and the saved tensor is not
modified in place.

MMIFunction / sMBRFunction (lattice-based, ops/ops.py:41-75,119-156) decode on the device
(lattice.MappedLatticeFasterRecognizer) and run the lattice forward-backward there; LatticeBatchFunction
is the whole-minibatch form.  MWEFunction (N-best minimum word error, ops/ops.py:158-241) and its minibatch form
MWEBatchFunction take the N best paths of the same device lattices.  TeacherStudentMMI (lattice teacher-student training,
ops/ops.py:77-117) and its minibatch form TeacherStudentBatch rescore the teacher's device lattices with the student.
"""
import numpy as np
import os

import torch
from torch.autograd import Function

from . import _lib, chain, ctc, lattice, transducer


class ChainObjtiveFunction(Function):
    """Per-utterance LF-MMI (the reference's spelling).  loglikes: [T', P] CUDA f32.  supervision: a chain.Supervision, or a
    chain.GraphSupervision of one utterance (alignment-free numerator)."""

    @staticmethod
    def forward(ctx, loglikes, den_graph, supervision, chain_opts):
        out, grad = chain.compute_chain_objf_and_deriv(chain_opts, den_graph, [supervision],
                                                       loglikes.detach().unsqueeze(0))
        ctx.save_for_backward(grad.squeeze(0))
        return out[0, 0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        grad_input, = ctx.saved_tensors
        return -grad_input, None, None, None


class ChainObjtiveBatch(Function):
    """All utterances of a minibatch in one call: prediction [B, T', P] (any strides with a unit
    pdf stride), supervisions = list of chain.Supervision, or one chain.GraphSupervision for the minibatch (alignment-free
    numerator; an utterance whose graph has no path of its length adds nothing).  Returns the summed objective, i.e.
    what the reference's per-utterance loop accumulates (bin/train_chain.py:261-275)."""

    @staticmethod
    def forward(ctx, prediction, den_graph, supervisions, chain_opts):
        # (round 6: the summed objective and the negated gradient come out of the library call -- out[0].sum() and
        # -grad_input were a reduction, two fills and a [N, T, P] elementwise kernel of torch's in the middle of every step)
        N = len(supervisions)
        out, neg_grad = chain.compute_chain_objf_and_deriv(chain_opts, den_graph, supervisions,
                                                           prediction.detach(), operator_form=True)
        ctx.save_for_backward(neg_grad)
        ctx.per_sequence = out[:3 * N].view(3, N)
        return out[3 * N]

    @staticmethod
    def backward(ctx, grad_out):
        neg_grad, = ctx.saved_tensors
        return neg_grad, None, None, None


class _CrossEntropyFunction(Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index, reduction):
        _lib.require_gpu()
        P = logits.shape[-1]
        x = logits.detach()
        # rows in memory order (works for the time-major views LSTMAM returns)
        if x.dim() == 3 and not x.is_contiguous() and x.transpose(0, 1).is_contiguous():
            x2 = x.transpose(0, 1).reshape(-1, P)
            tg = targets.transpose(0, 1).reshape(-1)
            layout = "tm"
        else:
            x2 = x.contiguous().view(-1, P)
            tg = targets.reshape(-1)
            layout = "bm"
        tg = tg.to(device=x.device, dtype=torch.int64).contiguous()
        rows = x2.shape[0]
        grad = torch.empty_like(x2)
        acc = torch.empty(2, dtype=torch.float32, device=x.device)
        cnt = acc[1:2].view(torch.int32)
        L = _lib.lib()
        # reduction='mean': the valid targets are counted by a one-workgroup launch in front, so the kernel writes the MEAN
        # loss's gradient as it is; backward applies the loss's incoming gradient in place by a launch that returns at
        # once when that gradient is exactly 1 (loss.backward()).  Rounds 1-6a scaled in a pass of its own over the
        # [rows, P] tensor (185 us of the 18.5 ms CE step for 2 x 470 MB; PK2_CE_SCALE_PASS=1 keeps it).
        ctx.prescaled = os.environ.get("PK2_CE_SCALE_PASS", "0") != "1"
        if reduction == "mean" and ctx.prescaled:
            _lib.check(L.pk2_softmax_ce_fwd_bwd_mean(_lib.ptr(x2), P, _lib.ptr(tg), int(ignore_index), rows, P,
                                                     _lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(grad), P, _lib.stream_ptr(x.device)))
        else:
            _lib.check(L.pk2_softmax_ce_fwd_bwd(_lib.ptr(x2), P, _lib.ptr(tg), int(ignore_index), rows, P,
                                                _lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(grad), P, None,
                                                _lib.stream_ptr(x.device)))
        if reduction == "mean":
            loss = acc[0] / cnt.to(torch.float32).clamp_min(1.0)[0]
        else:
            loss = acc[0].clone()
        ctx.save_for_backward(grad, cnt)
        ctx.mean = reduction == "mean"
        ctx.view = (layout, tuple(x.shape), P)
        ctx.applied = None          # the incoming gradient the saved buffer already carries (a second backward over a retained graph)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        grad, cnt = ctx.saved_tensors
        layout, shape, P = ctx.view
        go = grad_out.detach().to(device=grad.device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        if ctx.prescaled:
            _lib.check(_lib.lib().pk2_scale_inplace_ratio(_lib.ptr(grad), grad.numel(), _lib.ptr(go),
                                                          _lib.ptr(ctx.applied) if ctx.applied is not None else None,
                                                          _lib.stream_ptr(grad.device)))
            ctx.applied = go
            out = grad
        else:
            out = torch.empty_like(grad)
            _lib.check(_lib.lib().pk2_scale_by_scalars(_lib.ptr(grad), _lib.ptr(out), grad.numel(), _lib.ptr(go),
                                                       _lib.ptr(cnt) if ctx.mean else None, _lib.stream_ptr(grad.device)))
        g = out.view(shape[1], shape[0], P).transpose(0, 1) if layout == "tm" else out.view(shape)
        return g, None, None, None


class CrossEntropyLoss(torch.nn.Module):
    """nn.CrossEntropyLoss(ignore_index=-100, reduction='mean'|'sum') as the reference uses it
    (bin/train_ce.py:134,189; bin/train_se.py:214,235), fused into one HIP kernel."""

    def __init__(self, ignore_index=-100, reduction="mean"):
        super().__init__()
        assert reduction in ("mean", "sum")
        self.ignore_index, self.reduction = ignore_index, reduction

    def forward(self, logits, targets):
        return _CrossEntropyFunction.apply(logits, targets, self.ignore_index, self.reduction)


class MMIFunction(Function):
    """Lattice MMI for one utterance with the reference's signature (ops/ops.py:41-75):
    ``MMIFunction.apply(loglikes[T, P], asr_decoder, trans_model, trans_ids)``.  Forward returns the lattice
    log-likelihood (as the reference does); backward returns -(numerator - denominator posteriors)
    regardless of grad_out.  asr_decoder = lattice.MappedLatticeFasterRecognizer."""

    @staticmethod
    def forward(ctx, loglikes, asr_decoder, trans_model, trans_ids):
        lat = asr_decoder.decode(loglikes.detach().contiguous())
        like, post = lat.mmi([trans_ids], 1.0, 0.2, True)     # lattice_scale(1.0, 0.2), drop_frames, cancel
        ctx.save_for_backward(post[0])
        return like[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        return -post, None, None, None


class sMBRFunction(Function):
    """sMBR / MPFE for one utterance (ops/ops.py:119-156):
    ``sMBRFunction.apply(loglikes, asr_decoder, trans_model, trans_ids, criterion, silence_phones)``.
    Forward returns the expected frame accuracy; backward its negated derivative."""

    @staticmethod
    def forward(ctx, loglikes, asr_decoder, trans_model, trans_ids, criterion, silence_phones):
        lat = asr_decoder.decode(loglikes.detach().contiguous())
        score, post = lat.mpe([trans_ids], criterion, silence_phones, True)
        ctx.save_for_backward(post[0])
        return score[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        return -post, None, None, None, None, None


class LatticeBatchFunction(Function):
    """All utterances of a minibatch in one decode + one forward-backward launch: replaces the reference's
    per-utterance Python loop (bin/train_se.py:237-249).  prediction: [N, Tmax, P] log-likelihoods (log prior
    already subtracted); returns the summed criterion."""

    @staticmethod
    def forward(ctx, prediction, lengths, asr_decoder, trans_model, trans_ids, criterion, silence_phones):
        lat = asr_decoder.decode_batch(prediction.detach(), lengths)
        if criterion == "mmi":
            val, post = lat.mmi(trans_ids, 1.0, 0.2, True)
        else:
            val, post = lat.mpe(trans_ids, criterion, silence_phones, True)
        ctx.save_for_backward(post)
        ctx.per_sequence = val
        ctx.lattice = lat
        return val.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        return -post, None, None, None, None, None, None


class MWEFunction(Function):
    """N-best minimum word error for one utterance with the reference's signature (ops/ops.py:158-241):
    ``MWEFunction.apply(loglikes[T, P], asr_decoder, trans_model, supervision, config)``.  supervision = word ids, or
    with config['phone_level'] the transition-id alignment; config keys lm_weight, am_weight, phone_level, rand_path
    (must be false), num_paths (1..64), equal_weight, and optionally distinct.  Forward returns the expected edit
    distance; backward returns the saved gradient sum_k (e_k - loss) p_k per (frame, pdf of path k) regardless of
    grad_out, as the reference does."""

    @staticmethod
    def forward(ctx, loglikes, asr_decoder, trans_model, supervision, config):
        lattice.mwe_config(config)
        lat = asr_decoder.decode(loglikes.detach().contiguous())
        loss, grad = lat.mwe([supervision], config, trans_model)
        ctx.save_for_backward(grad[0])
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return grad, None, None, None, None


class MWEBatchFunction(Function):
    """MWE for all utterances of a minibatch in one decode and one N-best launch chain:
    ``MWEBatchFunction.apply(prediction[N, Tmax, P], lengths, asr_decoder, trans_model, supervisions, config)``.
    Returns the summed loss (float32); ctx.per_sequence holds the float64 loss of every utterance."""

    @staticmethod
    def forward(ctx, prediction, lengths, asr_decoder, trans_model, supervisions, config):
        lattice.mwe_config(config)
        lat = asr_decoder.decode_batch(prediction.detach(), lengths)
        loss, grad = lat.mwe(supervisions, config, trans_model)
        ctx.save_for_backward(grad)
        ctx.per_sequence = loss
        ctx.lattice = lat
        return loss.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return grad, None, None, None, None, None


class TeacherStudentMMI(Function):
    """Sequence-level distillation of a teacher into a student over the teacher's lattice, with the reference's signature
    (ops/ops.py:77-117): ``TeacherStudentMMI.apply(loglikes_T[T, P], loglikes_S[T, P], asr_decoder)``.  The lattice is decoded
    from the teacher's log-likelihoods, its posteriors are taken, it is rescored with the student's (old acoustic scores
    dropped) and its posteriors are taken again, on the unscaled lattice as in the reference (TeacherStudentBatch takes the
    scales).  Forward returns
    KL(P_T || P_S) over the lattice's paths as a 0-dim float32 tensor (the reference returned a Python float, and computed it
    as a cross-entropy of two Python lists); backward returns post_S - post_T for the student regardless of grad_out and
    None for the teacher (the reference returned post_T - post_S to an optimiser that minimises)."""

    @staticmethod
    def forward(ctx, loglikes_T, loglikes_S, asr_decoder):
        if loglikes_T.shape != loglikes_S.shape:
            raise ValueError("teacher and student log-likelihoods differ in shape: %s, %s" % (
                tuple(loglikes_T.shape), tuple(loglikes_S.shape)))
        lat = asr_decoder.decode(loglikes_T.detach().contiguous())
        loss, grad = lat.teacher_student(loglikes_S.detach().unsqueeze(0), 1.0, 1.0, 0.0)
        ctx.save_for_backward(grad[0])
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return None, grad, None


class TeacherStudentBatch(Function):
    """TeacherStudentMMI for all utterances of a minibatch in one decode and one launch chain:
    ``TeacherStudentBatch.apply(prediction_T[N, Tmax, P], prediction_S[N, Tmax, P], lengths, asr_decoder, lm_scale=1.0,
    acoustic_scale=1.0, old_acoustic_scale=0.0)``.  The two predictions agree in shape; their strides may differ (unit pdf
    stride).  Returns the summed loss (float32); ctx.per_sequence holds the float64 loss of every utterance, ctx.lattice the
    (rescored) lattices.  The gradient is that of the loss divided by acoustic_scale, as MMIFunction's."""

    @staticmethod
    def forward(ctx, prediction_T, prediction_S, lengths, asr_decoder, lm_scale=1.0, acoustic_scale=1.0,
                old_acoustic_scale=0.0):
        if prediction_T.shape != prediction_S.shape:
            raise ValueError("teacher and student predictions differ in shape: %s, %s" % (
                tuple(prediction_T.shape), tuple(prediction_S.shape)))
        lat = asr_decoder.decode_batch(prediction_T.detach(), lengths)
        loss, grad = lat.teacher_student(prediction_S.detach(), lm_scale, acoustic_scale, old_acoustic_scale)
        ctx.save_for_backward(grad)
        ctx.per_sequence = loss
        ctx.lattice = lat
        return loss.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return None, grad, None, None, None, None, None


class CTCFunction(Function):
    """``CTCFunction.apply(logits, lengths, labels, blank, reduction, zero_infinity, time_major)``: connectionist temporal
    classification on unnormalised logits [N, T, P] ([T, N, P] with time_major), ctc.ctc_loss_and_grad under autograd.  Forward
    computes loss and gradient in one library call with the reduction's factors as the per-utterance weights; backward hands
    the stored gradient on, multiplied by the incoming gradient only when that is not 1 (the CrossEntropyLoss scheme).
    ctx.per_sequence: float64 loss of every utterance, ctx.status: ctc.CTC_OK / CTC_NO_PATH / CTC_NUMERIC."""

    @staticmethod
    def forward(ctx, logits, lengths, labels, blank=0, reduction="mean", zero_infinity=True, time_major=False):
        N = len(labels)
        w = np.ones(N, np.float32)
        if reduction == "mean":
            w = (1.0 / (np.maximum([len(s) for s in labels], 1) * float(N))).astype(np.float32)
        loss, grad, status = ctc.ctc_loss_and_grad(logits, lengths, labels, blank, w, time_major)
        if not zero_infinity:      # an utterance without an alignment reports inf; its gradient rows stay 0
            loss = torch.where(status == ctc.CTC_NO_PATH, torch.full_like(loss, float("inf")), loss)
        ctx.per_sequence, ctx.status = loss, status
        ctx.save_for_backward(grad)
        ctx.utt_dim = None if reduction != "none" else (1 if time_major else 0)
        ctx.applied = None
        if reduction == "none":
            return loss.to(torch.float32)
        if reduction == "mean":
            loss = loss * _lib.h2d(w.astype(np.float64), loss.device)
        return loss.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        if ctx.utt_dim is not None:      # reduction 'none': one incoming gradient per utterance
            shape = [1, 1, 1]
            shape[ctx.utt_dim] = -1
            return (grad * grad_out.detach().to(torch.float32).view(shape),) + (None,) * 6
        go = grad_out.detach().to(device=grad.device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        _lib.check(_lib.lib().pk2_scale_inplace_ratio(_lib.ptr(grad), grad.numel(), _lib.ptr(go),
                                                      _lib.ptr(ctx.applied) if ctx.applied is not None else None,
                                                      _lib.stream_ptr(grad.device)))
        ctx.applied = go
        return (grad,) + (None,) * 6


class CTCLoss(torch.nn.Module):
    """torch.nn.CTCLoss(blank, reduction, zero_infinity) on UNNORMALISED logits, softmax included, fused into HIP kernels
    (csrc/ctc.hip): ``CTCLoss()(logits, lengths, labels)`` with logits [N, T, P] ([T, N, P] with time_major=True), lengths
    the frame counts and labels a list of int sequences.  'mean' divides every loss by its label count (at least 1) and
    averages over the utterances, 'sum' adds them, 'none' returns them.  zero_infinity (default True, unlike torch): an
    utterance with fewer frames than labels + repeats counts 0; with False it reports inf and still adds no gradient."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=True, time_major=False):
        super().__init__()
        assert reduction in ("mean", "sum", "none")
        self.blank, self.reduction, self.zero_infinity, self.time_major = blank, reduction, zero_infinity, time_major

    def forward(self, logits, lengths, labels):
        return CTCFunction.apply(logits, lengths, labels, self.blank, self.reduction, self.zero_infinity, self.time_major)


class TransducerFunction(Function):
    """``TransducerFunction.apply(am, lm, lengths, labels, blank, reduction, time_major, prune_range)``: the transducer loss with an additive
    joint on unnormalised logits am [N, T, V] ([T, N, V] with time_major) and lm [N, U + 1, V],
    transducer.transducer_loss_and_grad under autograd.  Forward computes the loss and both gradients in one library call
    with the reduction's factors as the per-utterance weights; backward hands the stored gradients on, multiplied by the
    incoming gradient only when that is not 1 (the CTCFunction scheme).  ctx.per_sequence: float64 loss of every utterance,
    ctx.status: transducer.TRANSDUCER_OK / TRANSDUCER_NUMERIC."""

    @staticmethod
    def forward(ctx, am, lm, lengths, labels, blank=0, reduction="mean", time_major=False, prune_range=None):
        N = len(labels)
        w = np.ones(N, np.float32)
        if reduction == "mean":
            w = (1.0 / (np.maximum([len(s) for s in labels], 1) * float(N))).astype(np.float32)
        begin = None
        if prune_range is None:
            loss, grad_am, grad_lm, status = transducer.transducer_loss_and_grad(am, lm, lengths, labels, blank, w, time_major)
        else:
            loss, grad_am, grad_lm, status, begin, _ = transducer.loss_grad_and_ranges(am, lm, lengths, labels, prune_range, blank, w,
                                                                                      time_major)
            ctx.mark_non_differentiable(begin)
        ctx.per_sequence, ctx.status = loss, status
        ctx.save_for_backward(grad_am, grad_lm)
        ctx.utt_dim = None if reduction != "none" else (1 if time_major else 0)
        ctx.applied = [None, None]
        if reduction == "none":
            out = loss.to(torch.float32)
        else:
            if reduction == "mean":
                loss = loss * _lib.h2d(w.astype(np.float64), loss.device)
            out = loss.sum().to(torch.float32)
        return out if begin is None else (out, begin)

    @staticmethod
    def backward(ctx, grad_out, *unused):
        grads = ctx.saved_tensors
        if ctx.utt_dim is not None:      # reduction 'none': one incoming gradient per utterance
            go = grad_out.detach().to(torch.float32)
            shape = [1, 1, 1]
            shape[ctx.utt_dim] = -1
            return (grads[0] * go.view(shape), grads[1] * go.view(-1, 1, 1)) + (None,) * 6
        go = grad_out.detach().to(device=grads[0].device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        for i, g in enumerate(grads):
            _lib.check(_lib.lib().pk2_scale_inplace_ratio(_lib.ptr(g), g.numel(), _lib.ptr(go),
                                                          _lib.ptr(ctx.applied[i]) if ctx.applied[i] is not None else None,
                                                          _lib.stream_ptr(g.device)))
            ctx.applied[i] = go
        return tuple(grads) + (None,) * 6


class TransducerLoss(torch.nn.Module):
    """The transducer (RNN-T) loss with an additive joint on UNNORMALISED logits, fused into HIP kernels that never store the
    joint (csrc/transducer.hip): ``TransducerLoss()(am, lm, lengths, labels)`` with am [N, T, V] ([T, N, V] with
    time_major=True), lm [N, U + 1, V] (row u: the predictor after u labels), lengths the frame counts and labels a list of
    int sequences.  'mean' divides every loss by its label count (at least 1) and averages over the utterances, 'sum' adds
    them, 'none' returns them.  With prune_range=S the call returns (loss, begin): begin int32 [N, T], not differentiable, the
    pruning ranges of transducer.loss_grad_and_ranges for PrunedJoin and PrunedTransducerLoss."""

    def __init__(self, blank=0, reduction="mean", time_major=False, prune_range=None):
        super().__init__()
        assert reduction in ("mean", "sum", "none")
        self.blank, self.reduction, self.time_major, self.prune_range = blank, reduction, time_major, prune_range

    def forward(self, am, lm, lengths, labels):
        return TransducerFunction.apply(am, lm, lengths, labels, self.blank, self.reduction, self.time_major, self.prune_range)


class PrunedTransducerFunction(Function):
    """``PrunedTransducerFunction.apply(logits, begin, lengths, labels, blank, reduction)``: the transducer loss on the 4-D logits
    [N, T, S, V] of a joiner evaluated on the band begin, transducer.pruned_loss_and_grad under autograd (the
    TransducerFunction scheme).  ctx.per_sequence: float64 loss of every utterance, ctx.status: transducer.TRANSDUCER_OK /
    TRANSDUCER_RANGES / TRANSDUCER_NUMERIC."""

    @staticmethod
    def forward(ctx, logits, begin, lengths, labels, blank=0, reduction="mean"):
        N = len(labels)
        w = np.ones(N, np.float32)
        if reduction == "mean":
            w = (1.0 / (np.maximum([len(s) for s in labels], 1) * float(N))).astype(np.float32)
        loss, grad, status = transducer.pruned_loss_and_grad(logits, begin, lengths, labels, blank, w)
        ctx.per_sequence, ctx.status = loss, status
        ctx.save_for_backward(grad)
        ctx.per_utt = reduction == "none"
        ctx.applied = None
        if reduction == "none":
            return loss.to(torch.float32)
        if reduction == "mean":
            loss = loss * _lib.h2d(w.astype(np.float64), loss.device)
        return loss.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        if ctx.per_utt:      # reduction 'none': one incoming gradient per utterance
            return (grad * grad_out.detach().to(torch.float32).view(-1, 1, 1, 1),) + (None,) * 5
        go = grad_out.detach().to(device=grad.device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        _lib.check(_lib.lib().pk2_scale_inplace_ratio(_lib.ptr(grad), grad.numel(), _lib.ptr(go),
                                                      _lib.ptr(ctx.applied) if ctx.applied is not None else None,
                                                      _lib.stream_ptr(grad.device)))
        ctx.applied = go
        return (grad,) + (None,) * 5


class PrunedTransducerLoss(torch.nn.Module):
    """The pruned transducer loss (k2's rnnt_loss_pruned) on the UNNORMALISED 4-D logits of a joiner, log-softmax included, in
    HIP (csrc/transducer_pruned.hip): ``PrunedTransducerLoss()(logits, begin, lengths, labels)`` with logits [N, T, S, V],
    row (t, s) for frame t and predictor row begin[t] + s, begin int32 [N, T] from TransducerLoss(prune_range=S).  The
    reductions are TransducerLoss's."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        assert reduction in ("mean", "sum", "none")
        self.blank, self.reduction = blank, reduction

    def forward(self, logits, begin, lengths, labels):
        return PrunedTransducerFunction.apply(logits, begin, lengths, labels, self.blank, self.reduction)


class PrunedJoin(Function):
    """``PrunedJoin.apply(enc, pred, begin, lengths, label_counts, S, tanh=True)``: h[n, t, s, :] = tanh(enc[n, t, :] +
    pred[n, begin[t] + s, :]) as [N, T, S, J], transducer.join_pruned under autograd: one launch forward, one backward, the
    gathered copies of enc and pred never made."""

    @staticmethod
    def forward(ctx, enc, pred, begin, lengths, label_counts, S, tanh=True):
        h = transducer.join_pruned(enc, pred, begin, lengths, label_counts, S, tanh)
        ctx.save_for_backward(h, begin)
        ctx.args = (list(lengths), list(label_counts), pred.shape[1], tanh)
        return h

    @staticmethod
    def backward(ctx, dh):
        h, begin = ctx.saved_tensors
        d_enc, d_pred = transducer.join_pruned_backward(dh, h, begin, *ctx.args)
        return (d_enc, d_pred) + (None,) * 5
