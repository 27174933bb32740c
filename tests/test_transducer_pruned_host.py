"""The pruned transducer, host side: the float64 restatement (tests/transducer_pruned_ref.py) pinned against the full-lattice
oracle of tests/transducer_ref.py and central differences; the band's invariants; the feasibility check of transducer.pack."""
import numpy as np
import pytest

from pykaldi2_amd import transducer

import transducer_pruned_ref as P
import transducer_ref as R


def test_a_band_that_holds_the_whole_lattice_equals_the_additive_oracle():
    rng = np.random.default_rng(0)
    T, U, V, S, blank = 5, 3, 6, 5, 2
    am, lm = 2.0 * rng.standard_normal((T, V)), 2.0 * rng.standard_normal((S, V))
    lab = rng.choice([v for v in range(V) if v != blank], size=U)
    loss, grad = P.pruned_loss_and_grad(am[:, None, :] + lm[None, :, :], np.zeros(T, int), lab, blank, 0.5)
    want, gam, glm = R.loss_and_grad(am, lm, lab, blank, 0.5)
    assert abs(loss - want) < 1e-12 and np.abs(grad.sum(1) - gam).max() < 1e-12 and np.abs(grad.sum(0)[:U + 1] - glm).max() < 1e-12
    assert not grad[:, U + 1:].any()


def test_central_differences_on_a_band():
    rng = np.random.default_rng(1)
    T, S, V, blank, lab, begin = 4, 2, 3, 0, [2, 1, 2], [0, 1, 1, 2]
    z = 2.0 * rng.standard_normal((T, S, V))
    loss, grad = P.pruned_loss_and_grad(z, begin, lab, blank)
    assert np.isfinite(loss) and np.abs(grad.sum(2)).max() < 1e-12
    h = 1e-5
    for i in np.ndindex(*z.shape):
        old = z[i]
        z[i] = old + h
        up = P.pruned_loss_and_grad(z, begin, lab, blank)[0]
        z[i] = old - h
        dn = P.pruned_loss_and_grad(z, begin, lab, blank)[0]
        z[i] = old
        assert abs((up - dn) / (2 * h) - grad[i]) < 1e-7


@pytest.mark.parametrize("T,U,S", [(1, 0, 2), (4, 3, 2), (3, 6, 4), (6, 2, 5), (9, 20, 5), (30, 7, 3), (12, 11, 2)])
def test_ranges_always_give_a_valid_band(T, U, S):
    Bmax = max(0, U + 1 - S)      # (4, 3, 2), (3, 6, 4) and (12, 11, 2): Bmax = (S - 1)(T - 1), exact feasibility
    assert Bmax <= (S - 1) * (T - 1)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        gamma = rng.random((T, U + 1)).astype(np.float32) ** (1 + seed)      # flat to peaked
        begin = P.ranges(gamma, T, U, S)
        steps = np.diff(begin)
        assert begin[0] == 0 and begin[-1] == Bmax and (steps >= 0).all() and (steps <= S - 1).all()


def test_pack_refuses_an_utterance_one_label_beyond_feasibility():
    T, S = 4, 3
    U = (S - 1) * (T - 1) + S - 1      # Bmax = (S - 1)(T - 1)
    transducer.pack([T], [[1] * U], T, U + 2, 5, prune_range=S)
    with pytest.raises(ValueError, match="utterance 0"):
        transducer.pack([T], [[1] * (U + 1)], T, U + 2, 5, prune_range=S)
    with pytest.raises(ValueError):
        transducer.pack([T], [[1]], T, 2, 5, prune_range=33)
