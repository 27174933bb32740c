"""Transducer loss, gradients and greedy decoding on the device (csrc/transducer.hip) against the float64 oracle of
tests/transducer_ref.py, which builds the 4-D joint, on the same float32 logits.  Tolerances are the project's for sequence
criteria: loss 1e-3 |want| + 1e-4, gradients 1e-4 absolute."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import _lib, ops, transducer

import transducer_ref as R

pytestmark = pytest.mark.gpu


def _poisoned(xs, V, time_major=False):
    """The utterances' rows inside a larger NaN-filled buffer, as [N, R, V] or [R, N, V]: non-trivial strides, poison beyond."""
    N, Rmax = len(xs), max(x.shape[0] for x in xs)
    big = torch.full((Rmax + 3, N, V + 9) if time_major else (N, Rmax + 3, V + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = big[:Rmax, :, 1:V + 1] if time_major else big[:, :Rmax, 1:V + 1]      # (rows start 4 bytes off a 16-byte boundary)
    for n, x in enumerate(xs):
        (view[:x.shape[0], n] if time_major else view[n, :x.shape[0]]).copy_(torch.from_numpy(x))
    return view


_want = {}      # oracle results by (case, utterance): computed once, shared


def _check(name, ams, lms, labels, blank=0, weights=None, time_major=False, status=None):
    """One call on the batch: loss, both gradients and status of every utterance against the oracle, zero rows past the
    lengths, a second call bit-identical.  Returns (loss, grad_am [N, T, V], grad_lm, status) as numpy arrays."""
    V, frames = ams[0].shape[1], [x.shape[0] for x in ams]
    am, lm = _poisoned(ams, V, time_major), _poisoned(lms, V)
    out = [transducer.transducer_loss_and_grad(am, lm, frames, labels, blank, weights, time_major) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out)) and out[0][1].shape == am.shape and out[0][2].shape == lm.shape
    loss, gam, glm, st = [o.cpu().numpy() for o in out[0]]
    gam = gam.transpose(1, 0, 2) if time_major else gam
    assert st.tolist() == (status or [0] * len(ams))
    for n, lab in enumerate(labels):
        T, U1 = frames[n], len(lab) + 1
        assert not gam[n, T:].any() and not glm[n, U1:].any()
        if st[n]:
            assert loss[n] == 0.0 and not gam[n].any() and not glm[n].any()
            continue
        w = 1.0 if weights is None else float(np.float32(weights[n]))
        if (name, n) not in _want:
            _want[name, n] = R.loss_and_grad(ams[n], lms[n], lab, blank)
        want_loss, want_am, want_lm = _want[name, n]
        err = abs(loss[n] - want_loss), np.abs(gam[n, :T] - w * want_am).max(), np.abs(glm[n, :U1] - w * want_lm).max()
        print("%s utt %d: T %d U %d V %d loss %.6f want %.6f (err %.3g) grad_am err %.3g grad_lm err %.3g row sums %.3g"
              % ((name, n, T, U1 - 1, V, loss[n], want_loss) + err + (np.abs(gam[n].sum(1)).max(),)))
        assert err[0] <= 1e-3 * abs(want_loss) + 1e-4 and err[1] <= 1e-4 and err[2] <= 1e-4
    return loss, gam, glm, st


#        name: (V, blank, [(T, U), ..], logit scale)
_CASES = {"edges": (7, 0, [(1, 0), (1, 5), (6, 0), (4, 3)], 2.0),               # one cell, one row, one column
          "thin": (7, 3, [(3, 40), (40, 3)], 2.0),                               # T < U and T > U, the blank in the middle
          "waves": (5, 4, [(3, 62), (3, 63), (3, 64)], 2.0),                     # U + 1 = 63, 64, 65: the exchange crosses waves
          "limit": (5, 0, [(2, transducer.MAX_LABELS)], 2.0),                    # a workgroup of 1024 lanes
          "V2": (2, 0, [(5, 3)], 2.0),                                           # all labels equal
          "V43": (43, 42, [(20, 6)], 2.0),
          "V31": (31, 0, [(9, 4)], 2.0), "V33": (33, 0, [(9, 4)], 2.0),          # the K tile of the normaliser is 32
          "V5768": (5768, 5767, [(33, 17)], 2.0),
          "tile65": (9, 0, [(65, 64)], 2.0),                                     # T and U + 1 one above the 64 x 64 output tile
          "repeats": (6, 2, [(7, 5), (7, 5)], 2.0),                              # all equal / a a b a a
          "ragged": (23, 7, [(21, 2), (76, 9), (80, 10), (22, 2)], 2.0),         # 146 / 539 / 569 / 159 frames scaled to T <= 80
          "spread": (40, 0, [(12, 5), (9, 11)], None),                           # every row of am and of lm scaled to max - min = 30
          "long": (10, 0, [(300, 120)], 3.0)}                                    # peaked: the loss is of the order 10^3


def _case(name):
    V, blank, shapes, scale = _CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    cols = np.array([v for v in range(V) if v != blank])
    labels = [cols[rng.integers(0, len(cols), size=U)].tolist() for _, U in shapes]
    if name == "repeats":
        labels = [[4] * 5, [1, 1, 3, 1, 1]]
    mk = lambda rows: ((scale or 1.0) * rng.standard_normal((rows, V))).astype(np.float32)      # noqa: E731
    ams, lms = [mk(T) for T, _ in shapes], [mk(U + 1) for _, U in shapes]
    if scale is None:
        ams, lms = [[(x * (30.0 / (x.max(1, keepdims=True) - x.min(1, keepdims=True)))).astype(np.float32) for x in xs] for xs in (ams, lms)]
    kw = dict(blank=blank, weights=[0.5, 2.0, 0.125, 1.75] if name == "ragged" else None)
    return ams, lms, labels, kw


@pytest.mark.parametrize("name,time_major", [(n, False) for n in _CASES] + [(n, True) for n in ("edges", "waves", "V5768", "ragged")])
def test_parity_with_the_oracle(name, time_major):
    ams, lms, labels, kw = _case(name)
    _check(name, ams, lms, labels, time_major=time_major, **kw)


def test_an_utterance_alone_is_bit_identical_to_its_rows_in_the_batch():
    ams, lms, labels, kw = _case("ragged")
    loss, gam, glm, _ = _check("ragged", ams, lms, labels, **kw)
    for n in range(4):
        l1, a1, g1, _ = _check("ragged%d" % n, [ams[n]], [lms[n]], [labels[n]], blank=kw["blank"], weights=[kw["weights"][n]])
        T, U1 = ams[n].shape[0], len(labels[n]) + 1
        assert l1[0].tobytes() == loss[n].tobytes()
        assert np.array_equal(a1[0].view(np.int32), gam[n, :T].view(np.int32)) and np.array_equal(g1[0].view(np.int32), glm[n, :U1].view(np.int32))


def test_outside_the_range_is_status_3_and_leaves_the_neighbours_alone():
    """am rows of +200 in column 1 and -200 elsewhere against lm rows of +200 in column 2: every product exp(am - max)
    exp(lm - max) is 0 in float32 (checked here before relying on it), so S = 0."""
    ams, lms, labels, kw = _case("ragged")
    bad_am, bad_lm = np.full((9, 23), -200.0, np.float32), np.full((4, 23), -200.0, np.float32)
    bad_am[:, 1], bad_lm[:, 2] = 200.0, 200.0
    assert not R.normaliser_f32(bad_am, bad_lm).any()
    loss, gam, glm, _ = _check("st3", [ams[0], bad_am, ams[2]], [lms[0], bad_lm, lms[2]], [labels[0], [5, 6, 5], labels[2]], blank=7,
                               status=[0, 3, 0])
    loss2, gam2, glm2, _ = _check("st3b", [ams[0], ams[2]], [lms[0], lms[2]], [labels[0], labels[2]], blank=7)
    for a, b in ((0, 0), (2, 1)):
        assert loss[a].tobytes() == loss2[b].tobytes() and np.array_equal(gam[a].view(np.int32), gam2[b].view(np.int32))
        assert np.array_equal(glm[a].view(np.int32), glm2[b].view(np.int32))


def test_workspace_has_no_term_in_T_U_V():
    T, U = 64, 31
    host = torch.from_numpy(transducer.pack([T], [[1] * U], T, U + 1, 43))
    small, large = [_lib.lib().pk2_transducer_workspace_bytes(_lib.ptr(host), 1, V) for V in (43, 5768)]
    assert small > 0 and large - small <= 4 * 4 * (T + U + 1) * (5768 - 43)


@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_transducer_loss_under_autograd(reduction):
    ams, lms, labels, kw = _case("ragged")
    frames = [x.shape[0] for x in ams]
    am, lm = [_poisoned(xs, 23).clone().requires_grad_() for xs in (ams, lms)]
    out = ops.TransducerLoss(kw["blank"], reduction)(am, lm, frames, labels)
    assert out.grad_fn.per_sequence.dtype == torch.float64 and out.grad_fn.per_sequence.shape == (4,)
    (out * 0.5).sum().backward()
    w = [{"sum": 1.0, "none": 1.0, "mean": 1.0 / (4 * max(len(lab), 1))}[reduction] for lab in labels]
    want = [R.loss_and_grad(a, p, lab, kw["blank"], 0.5 * wn) for a, p, lab, wn in zip(ams, lms, labels, w)]
    losses = np.array([wn * x[0] for wn, x in zip(w, want)])
    got, want_out = out.detach().cpu().numpy(), (losses if reduction == "none" else losses.sum())
    assert (np.abs(got - want_out) <= 1e-3 * np.abs(want_out) + 1e-4).all()
    for n, (_, ga, gl) in enumerate(want):
        assert np.abs(am.grad[n, :frames[n]].cpu().numpy() - ga).max() <= 1e-4 and np.abs(lm.grad[n, :gl.shape[0]].cpu().numpy() - gl).max() <= 1e-4


@pytest.mark.parametrize("case", ["seed0", "seed1", "seed2", "seed3", "seed4", "cut", "tie"])
def test_greedy_decode_equals_the_restatement(case):
    rng = np.random.default_rng(sum(map(ord, case)))
    V, blank, frames, max_symbols = 70, 69, [9, 1, 14], 8
    table = rng.standard_normal((V, V)).astype(np.float32)
    ams = [(2.0 * rng.standard_normal((T, V))).astype(np.float32) for T in frames]
    if case == "cut":          # every row prefers a non-blank column: each frame emits max_symbols tokens
        table[:, blank], max_symbols = -100.0, 3
    elif case == "tie":        # small integers: the sums are exact, columns 5 and 40 tie for the maximum of every row
        table, ams = np.zeros((V, V), np.float32), [rng.integers(-8, 8, size=(T, V)).astype(np.float32) for T in frames]
        for x in ams:
            x[:, 5] = x[:, 40] = 9.0
        table[5, blank] = 32.0
    got = transducer.greedy_decode(_poisoned(ams, V), frames, _poisoned([table], V)[0], blank, max_symbols)
    want = [R.greedy(x, table, blank, max_symbols) for x in ams]
    assert got == want and any(want)
    assert case != "cut" or [len(h) for h in want] == [3 * T for T in frames]
    assert case != "tie" or want[1] == [5]
