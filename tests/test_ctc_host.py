"""CTC, host side: the float64 oracle (tests/ctc_ref.py) pinned against an enumeration of every alignment and against
torch.nn.functional.ctc_loss in float64 on the CPU; the argument checks of ctc.ctc_loss_and_grad, which precede any launch."""
import itertools

import numpy as np
import pytest
import torch

from pykaldi2_amd import ctc

import ctc_ref as R


def _collapse(path, blank):
    return [k for k, _ in itertools.groupby(path) if k != blank]


@pytest.mark.parametrize("blank", [0, 2])
def test_oracle_equals_the_sum_over_all_alignments(blank):
    rng = np.random.default_rng(1)
    P, syms = 3, [k for k in range(3) if k != blank]
    for T in range(1, 7):
        x = 2.0 * rng.standard_normal((T, P))
        logy = x - np.log(np.exp(x).sum(1, keepdims=True))
        total = {}
        for path in itertools.product(range(P), repeat=T):
            key = tuple(_collapse(path, blank))
            total[key] = total.get(key, 0.0) + np.exp(logy[np.arange(T), list(path)].sum())
        for L in range(4):
            for lab in itertools.product(syms, repeat=L):
                loss, grad, status = R.loss_and_grad(x, lab, blank)
                if lab not in total:
                    assert status == 2 and loss == 0.0 and not grad.any()
                else:
                    assert status == 0 and abs(loss + np.log(total[lab])) < 1e-10 and np.abs(grad.sum(1)).max() < 1e-10


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_oracle_equals_torch_float64(reduction):
    rng = np.random.default_rng(2)
    P, blank = 7, 3
    frames, labels = [9, 14, 5, 6], [[1, 1, 2], [0, 4, 4, 6, 5, 1], [], [2, 2, 2, 2]]      # the last one has no alignment
    N, Tmax = len(frames), max(frames)
    x = torch.tensor(rng.standard_normal((N, Tmax, P)) * 3.0, dtype=torch.float64, requires_grad=True)
    tgt = torch.tensor([lab + [0] * (6 - len(lab)) for lab in labels])
    out = torch.nn.functional.ctc_loss(x.log_softmax(2).transpose(0, 1), tgt, torch.tensor(frames), torch.tensor([len(s) for s in labels]),
                                       blank=blank, reduction=reduction, zero_infinity=True)
    go = torch.tensor(rng.random(N) + 0.5) if reduction == "none" else torch.tensor(1.0)
    (out * go).sum().backward()
    w = go.numpy() if reduction == "none" else np.full(N, 1.0) if reduction == "sum" else 1.0 / (np.maximum([len(s) for s in labels], 1) * N)
    got = [R.loss_and_grad(x.detach().numpy()[n, :T], lab, blank, w[n]) for n, (T, lab) in enumerate(zip(frames, labels))]
    assert [g[2] for g in got] == [0, 0, 0, 2]
    losses = np.array([g[0] for g in got])
    want = out.detach().numpy()
    assert np.abs((losses if reduction == "none" else (losses * w).sum()) - want).max() < 1e-9
    for n, T in enumerate(frames):
        assert np.abs(got[n][1] - x.grad.numpy()[n, :T]).max() < 1e-9 and not x.grad.numpy()[n, T:].any()


@pytest.mark.parametrize("bad", ["blank_in_labels", "too_long", "length_beyond_tensor"])
def test_bad_arguments_raise_before_any_launch(bad):
    x = torch.zeros(2, 8, 5)
    lengths, labels = [8, 6], [[1, 2], [3]]
    if bad == "blank_in_labels":
        labels[1] = [3, 0]
    elif bad == "too_long":
        labels[0] = [1, 2] * 2048
    else:
        lengths[1] = 9
    with pytest.raises(ValueError):
        ctc.ctc_loss_and_grad(x, lengths, labels, blank=0)
    assert ctc.pack([8, 6], [[1, 2], [3]], 8, 5)[:8].tolist() == [8, 2, 0, 16, 18, 0x3f800000, 0, 0]
