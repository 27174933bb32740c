"""Transducer, host side: the float64 oracle (tests/transducer_ref.py) pinned against an enumeration of every alignment and
against central differences; the argument checks of transducer.pack, which precede any launch."""
import itertools

import numpy as np
import pytest
import torch

from pykaldi2_amd import transducer

import transducer_ref as R


def _inputs(T, U, V=4, blank=1, seed=0):
    rng = np.random.default_rng(seed + 10 * T + U)
    lab = rng.choice([v for v in range(V) if v != blank], size=U)
    return 2.0 * rng.standard_normal((T, V)), 2.0 * rng.standard_normal((U + 1, V)), lab, blank


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (3, 0), (3, 2), (2, 3)])
def test_oracle_equals_the_sum_over_all_alignments_and_central_differences(T, U):
    am, lm, lab, blank = _inputs(T, U)
    loss, gam, glm = R.loss_and_grad(am, lm, lab, blank)
    logy = R.lattice(am, lm, lab, blank)[1]
    total = 0.0
    for moves in set(itertools.permutations([0] * (T - 1) + [1] * U)):      # 0: blank (t + 1), 1: label (u + 1); then the last blank
        t = u = 0
        lp = 0.0
        for mv in moves:
            lp += logy[t, u, lab[u]] if mv else logy[t, u, blank]
            t, u = t + 1 - mv, u + mv
        total += np.exp(lp + logy[t, u, blank])
    assert abs(loss + np.log(total)) < 1e-10 and np.abs(gam.sum(1)).max() < 1e-10
    h = 1e-5
    for x, g in ((am, gam), (lm, glm)):
        for i in np.ndindex(*x.shape):
            old = x[i]
            x[i] = old + h
            up = R.loss_and_grad(am, lm, lab, blank)[0]
            x[i] = old - h
            dn = R.loss_and_grad(am, lm, lab, blank)[0]
            x[i] = old
            assert abs((up - dn) / (2 * h) - g[i]) < 1e-7


@pytest.mark.parametrize("bad", ["blank_in_labels", "label_out_of_range", "too_many_labels", "length_zero", "length_beyond_tensor",
                                 "too_few_lm_rows", "dtype", "stride"])
def test_bad_arguments_raise_before_any_launch(bad):
    am, lm = torch.zeros(2, 8, 5), torch.zeros(2, 3, 5)
    lengths, labels = [8, 6], [[1, 2], [3]]
    if bad == "blank_in_labels":
        labels[1] = [0]
    elif bad == "label_out_of_range":
        labels[1] = [5]
    elif bad == "too_many_labels":
        labels[0], lm = [1] * (transducer.MAX_LABELS + 1), torch.zeros(2, transducer.MAX_LABELS + 2, 5)
    elif bad == "length_zero":
        lengths[1] = 0
    elif bad == "length_beyond_tensor":
        lengths[1] = 9
    elif bad == "too_few_lm_rows":
        labels[0] = [1, 2, 3]
    elif bad == "dtype":
        lm = lm.double()
    else:
        am = torch.zeros(2, 8, 10)[:, :, ::2]
    with pytest.raises(ValueError):
        transducer.transducer_loss_and_grad(am, lm, lengths, labels, blank=0)
    assert transducer.pack([8, 6], [[1, 2], [3]], 8, 3, 5)[:8].tolist() == [8, 2, 0, 16, 18, 0x3f800000, 0, 0]
