"""CTC loss and gradient on the device (csrc/ctc.hip) against the float64 oracle of tests/ctc_ref.py on the same float32
logits.  Tolerances are the chain path's (tests/test_gpu_chain.py): loss 1e-3 |want| + 1e-4, gradients 1e-4 absolute."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import ctc, ops

import ctc_ref as R

pytestmark = pytest.mark.gpu


def _labels(rng, L, P, blank, same=()):
    """L labels, none the blank, no two neighbours equal except lab[i] == lab[i - 1] for i in `same`."""
    cols = np.array([k for k in range(P) if k != blank])
    idx = np.cumsum(rng.integers(1, max(len(cols) - 1, 1) + 1, size=L)) % len(cols) if len(cols) > 1 else np.zeros(L, int)
    lab = cols[idx]
    for i in same:
        lab[i] = lab[i - 1]
        assert i + 1 >= L or lab[i + 1] != lab[i]
    return lab.tolist()


def _poisoned(xs, P, time_major):
    """The utterances' logits inside a larger NaN-filled buffer, as [N, T, P] or [T, N, P]: non-trivial strides, poison beyond."""
    N, Tmax = len(xs), max(x.shape[0] for x in xs)
    big = torch.full((Tmax + 3, N, P + 9) if time_major else (N, Tmax + 3, P + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = big[:Tmax, :, :P] if time_major else big[:, :Tmax, :P]
    for n, x in enumerate(xs):
        (view[:x.shape[0], n] if time_major else view[n, :x.shape[0]]).copy_(torch.from_numpy(x))
    return view


_want = {}      # oracle results by (case, utterance): computed once, shared


def _check(name, xs, labels, blank=0, weights=None, time_major=False, status=None):
    """One call on the batch: loss, gradient and status of every utterance against the oracle, zero rows past the lengths,
    a second call bit-identical.  Returns (loss, grad [N, T, P], status) as numpy arrays."""
    P, frames = xs[0].shape[1], [x.shape[0] for x in xs]
    x = _poisoned(xs, P, time_major)
    out = [ctc.ctc_loss_and_grad(x, frames, labels, blank, weights, time_major) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out)) and out[0][1].shape == x.shape
    loss, grad, st = [o.cpu().numpy() for o in out[0]]
    grad = grad.transpose(1, 0, 2) if time_major else grad
    assert st.tolist() == (status or [0] * len(xs))
    for n, (xn, lab) in enumerate(zip(xs, labels)):
        w = 1.0 if weights is None else float(np.float32(weights[n]))
        if (name, n) not in _want:
            _want[name, n] = R.loss_and_grad(xn, lab, blank)
        want_loss, want_grad, want_st = _want[name, n]
        err_l, err_g = abs(loss[n] - want_loss), np.abs(grad[n, :frames[n]] - w * want_grad).max()
        print("%s utt %d: T %d L %d loss %.6f want %.6f (err %.3g) grad err %.3g" % (name, n, frames[n], len(lab), loss[n], want_loss, err_l, err_g))
        assert st[n] == want_st and err_l <= 1e-3 * abs(want_loss) + 1e-4 and err_g <= 1e-4
        assert not grad[n, frames[n]:].any()
    return loss, grad, st


def _case(name):
    """(xs, labels, kwargs) of a named case: seeded, the smallest shapes at which each part of the kernels can go wrong."""
    rng = np.random.default_rng(sum(map(ord, name)))
    mk = lambda T, P, scale=2.0: (scale * rng.standard_normal((T, P))).astype(np.float32)      # noqa: E731
    kw = {}
    if name.startswith("tiny"):          # the blank-only pair, the final sum over one state
        P, blank = 5, (4 if name.endswith("last") else 0)
        frames, labels, kw = [1, 1, 5], [[], [2], []], dict(blank=blank)
    elif name == "wave_boundary":        # pair 64 is lane 0 of the second wave: the neighbour value and the skip bit cross waves
        P, labels = 40, [_labels(rng, 63, 40, 0), _labels(rng, 64, 40, 0), _labels(rng, 65, 40, 0), _labels(rng, 65, 40, 0, same=[64])]
        frames = [70, 64, 75, 66]       # (64 = L and 66 = L + 1 repeat: exactly the minimum)
    elif name == "two_pairs":            # 512 -> 513 pairs: one -> two pairs per lane
        P, labels, frames = 40, [_labels(rng, L, 40, 39) for L in (511, 512, 513)], [611, 612, 613]
        kw = dict(blank=39)
    elif name == "limit":                # L = 4095: 8 pairs per lane
        P, labels, frames = 40, [_labels(rng, 4095, 40, 0)], [4195]
    elif name in ("P2", "P61", "P5768"):
        P = int(name[1:])
        labels, frames = ([[1, 1, 1]], [8]) if P == 2 else ([_labels(rng, 10, P, P - 1)], [50])
        kw = dict(blank=0 if P == 2 else P - 1)
    elif name == "spread80":             # every row scaled to max - min = 80
        P, labels, frames = 40, [_labels(rng, 12, 40, 0), _labels(rng, 30, 40, 0, same=[7])], [60, 33]
    elif name == "long_blank_runs":      # where the log scale accumulates
        P, labels, frames = 40, [_labels(rng, 5, 40, 0)], [3000]
    else:                                # "ragged": four lengths, weights other than 1
        P, labels, frames = 23, [_labels(rng, L, 23, 7) for L in (9, 0, 31, 4)], [40, 7, 33, 19]
        kw = dict(blank=7, weights=[0.5, 2.0, 0.125, 1.75])
    xs = [mk(T, P) for T in frames]
    if name == "spread80":
        xs = [(x * (80.0 / (x.max(1, keepdims=True) - x.min(1, keepdims=True)))).astype(np.float32) for x in xs]
    return xs, labels, kw


@pytest.mark.parametrize("name,time_major", [(n, False) for n in ("tiny", "tiny_blank_last", "wave_boundary", "two_pairs", "limit", "P2",
                                                                   "P61", "P5768", "spread80", "long_blank_runs", "ragged")] +
                         [(n, True) for n in ("tiny", "wave_boundary", "P5768", "ragged")])      # [T, N, P]: the strides differ only
def test_parity_with_the_oracle(name, time_major):
    xs, labels, kw = _case(name)
    _check(name, xs, labels, time_major=time_major, **kw)


def test_repeats_at_the_minimum_length_and_below():
    """a a b b b c needs 6 + 3 frames: at 9 there is one alignment (the gradient is y minus 0 / 1), at 8 none: status 2 and
    zeros, the neighbours bit-identical to the batch without it."""
    xs, labels, _ = _case("ragged")
    lab = [1, 1, 2, 2, 2, 3]
    rng = np.random.default_rng(5)
    x9, x8 = [rng.standard_normal((T, 23)).astype(np.float32) for T in (9, 8)]
    loss, grad, _ = _check("min", [xs[0], x9, x8, xs[2]], [labels[0], lab, lab, labels[2]], blank=7, status=[0, 0, 2, 0])
    y = torch.from_numpy(x9).double().softmax(1).numpy()
    occ = y - grad[1, :9]
    assert np.abs(occ - np.round(occ)).max() <= 1e-4 and np.abs(occ.sum(1) - 1.0).max() <= 1e-4
    assert loss[2] == 0.0 and not grad[2].any()
    loss2, grad2, _ = _check("min2", [xs[0], x9, xs[2]], [labels[0], lab, labels[2]], blank=7)
    for a, b in ((0, 0), (1, 1), (3, 2)):
        assert loss[a].tobytes() == loss2[b].tobytes() and np.array_equal(grad[a].view(np.int32), grad2[b].view(np.int32))


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_ctc_loss_under_autograd(reduction):
    """ops.CTCLoss through a Linear against torch's CTC in float64 on the CPU; with zero_infinity=False the utterance
    without an alignment reports inf and the others' gradients do not change."""
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    F, P, blank, frames = 16, 11, 10, [30, 12, 4, 21]
    labels = [_labels(rng, 8, P, blank), [], [3, 3, 3], _labels(rng, 20, P, blank)]      # the third has no alignment
    lin = torch.nn.Linear(F, P).cuda()
    feats = torch.randn(4, 30, F, device="cuda")
    go = torch.tensor(rng.random(4) + 0.5, dtype=torch.float32) if reduction == "none" else torch.tensor(1.0)
    got = {}
    for zero_inf in (True, False):
        lin.zero_grad()
        out = ops.CTCLoss(blank, reduction, zero_infinity=zero_inf)(lin(feats), frames, labels)
        ((out * go.cuda())[torch.isfinite(out)] if reduction == "none" else out).sum().backward()
        got[zero_inf] = (out.detach().cpu().double(), lin.weight.grad.cpu().double().clone())
    ref = torch.nn.Linear(F, P).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in lin.state_dict().items()})
    tgt = torch.tensor([lab + [0] * (20 - len(lab)) for lab in labels])
    want = torch.nn.functional.ctc_loss(ref(feats.cpu().double()).log_softmax(2).transpose(0, 1), tgt, torch.tensor(frames),
                                        torch.tensor([len(s) for s in labels]), blank=blank, reduction=reduction, zero_infinity=True)
    (want * go.double()).sum().backward()
    # |d W[k, f]| error <= sum over the frames of (1e-4 on the logits' gradient) |feat[., f]|, times the largest weight
    tol_w = 1e-4 * float(feats.abs().sum((0, 1)).max()) * float(go.max())
    print("loss", got[True][0], "want", want.detach(), "dW err %.3g (tol %.3g)" % ((got[True][1] - ref.weight.grad).abs().max(), tol_w))
    assert ((got[True][0] - want.detach()).abs() <= 1e-3 * want.detach().abs() + 1e-4).all()
    assert (got[True][1] - ref.weight.grad).abs().max() <= tol_w
    assert torch.equal(got[False][1], got[True][1])
    if reduction == "none":
        assert torch.isinf(got[False][0][2]) and torch.equal(got[False][0][[0, 1, 3]], got[True][0][[0, 1, 3]])
    else:
        assert torch.isinf(got[False][0])
