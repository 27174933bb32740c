"""Float64 oracle of the fused softmax cross-entropy of include/pk2hip.h (pk2_softmax_ce_fwd_bwd, _mean; csrc/softmax_ce.hip),
numpy only -- TEST INFRASTRUCTURE ONLY.

Written from the definition of nn.CrossEntropyLoss(ignore_index, reduction) plus the two rules of the library's own:

  * a row whose target is neither ignore_index nor inside [0, P) never indexes the row: it adds NaN to the loss, its
    gradient is zero and it is not counted (nn.CrossEntropyLoss asserts there);
  * the mean divides by max(1, count), so a call with every target ignored gives loss 0 and gradient 0.

log_softmax_model restates the two float32 formulas a kernel can use for the log-probabilities (the maximum subtracted
first, or a log-sum-exp subtracted from the raw logit): the CPU model the bounds of tests/edge_cases.py, applied by
tests/test_gpu_ce_optim_frontend.py, are calibrated with.
"""
import numpy as np


def log_softmax64(x):
    """log softmax over the last axis in float64 (-inf logits allowed, not a whole row of them)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = x.max(axis=-1, keepdims=True)
        d = x - m
        return d - np.log(np.exp(d).sum(axis=-1, keepdims=True))


def valid_rows(targets, num_classes, ignore_index=-100):
    """(valid, out_of_range): bool [rows] each."""
    t = np.asarray(targets, dtype=np.int64)
    oor = (t != ignore_index) & ((t < 0) | (t >= num_classes))
    return (t != ignore_index) & ~oor, oor


def cross_entropy(x, targets, ignore_index=-100, reduction="mean"):
    """x: [rows, P] float32, targets: [rows] int64.  Returns (loss_sum, count, grad, logprob) in float64:
    loss_sum = sum of the valid rows' -logprob[target] (NaN when a target is out of range), count = valid rows,
    grad = d loss / d x of the reduction ('sum', or 'mean' = sum / max(1, count)), logprob = log_softmax64(x) of EVERY row."""
    assert reduction in ("mean", "sum")
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    rows, P = x.shape
    t = np.asarray(targets, dtype=np.int64)
    valid, oor = valid_rows(t, P, ignore_index)
    lp = log_softmax64(x)
    r = np.nonzero(valid)[0]
    loss_sum = float(-lp[r, t[r]].sum())
    if oor.any():
        loss_sum = float("nan")
    count = int(valid.sum())
    grad = np.zeros((rows, P), dtype=np.float64)
    grad[r] = np.exp(lp[r])
    grad[r, t[r]] -= 1.0
    if reduction == "mean":
        grad /= max(1, count)
    return loss_sum, count, grad, lp


def reduce_loss(loss_sum, count, reduction):
    return loss_sum / max(1, count) if reduction == "mean" else loss_sum


def log_softmax_model(x, max_first, dtype=np.float32):
    """The log-probabilities as a kernel computes them, every operation rounded to `dtype`:
    max_first: (x - m) - log(s);   otherwise: x - (m + log(s)),    m = max x, s = sum exp(x - m)."""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(invalid="ignore"):
        m = x.max(axis=-1, keepdims=True)
        s = np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)
        if max_first:
            return (x - m) - np.log(s)
        return x - (m + np.log(s))


def softmax_grad_model(x, targets, max_first, dtype=np.float32):
    """exp(log_softmax_model) - onehot, the gradient the streaming kernel writes, in `dtype`."""
    g = np.exp(log_softmax_model(x, max_first, dtype))
    g[np.arange(g.shape[0]), np.asarray(targets)] -= dtype(1)
    return g
