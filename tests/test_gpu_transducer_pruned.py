"""The pruned transducer on the device (csrc/transducer_pruned.hip) against the float64 restatement of
tests/transducer_pruned_ref.py on the same float32 inputs.  Tolerances are the project's for sequence criteria (DESIGN.md
7.19): loss 1e-3 |want| + 1e-4, gradients and gamma 1e-4 absolute; the join's is measured in its test."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import _lib, ops, transducer

import transducer_pruned_ref as P
import transducer_ref as R
from test_gpu_transducer import _poisoned

pytestmark = pytest.mark.gpu


def _poisoned4(xs):
    """[T, S, V] arrays inside a larger NaN-filled [N, T + 2, S + 1, V + 9] buffer: odd strides, rows 4 bytes off 16."""
    (S, V), Tmax = xs[0].shape[1:], max(x.shape[0] for x in xs)
    big = torch.full((len(xs), Tmax + 2, S + 1, V + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = big[:, :Tmax, :S, 1:V + 1]
    for n, x in enumerate(xs):
        view[n, :x.shape[0]].copy_(torch.from_numpy(x))
    return view


def _band(kind, T, U, S, rng):
    if kind == "random":
        return P.ranges(rng.random((T, U + 1)) ** 8, T, U, S)
    return np.arange(T) * ((S - 1) if kind == "full" else 0)


def _begin(bands):
    out = np.full((len(bands), max(len(b) for b in bands)), -7, np.int32)      # entries past T_n are never read
    for n, b in enumerate(bands):
        out[n, :len(b)] = b
    return torch.from_numpy(out).cuda()


#        name: (V, blank, S, [(T, U, band), ..])
_CASES = {"zero": (7, 0, 5, [(63, 4, "zero")]),
          "full": (2, 0, 2, [(64, 64, "full")]),                       # a step of S - 1 at every frame; all labels equal
          "random": (31, 15, 5, [(65, 40, "random")]),
          "U0": (33, 32, 32, [(130, 0, "zero")]),
          "S32": (43, 42, 32, [(130, 100, "random")]),
          "V5768": (5768, 5767, 2, [(5, 3, "random")]),
          "below": (transducer.PRUNED_SHORT_ROWS - 1, 0, 5, [(9, 6, "random")]),
          "at": (transducer.PRUNED_SHORT_ROWS, 0, 5, [(9, 6, "random")]),
          "ragged": (23, 7, 5, [(21, 2, "zero"), (76, 9, "random"), (80, 10, "random"), (10, 40, "full")])}
_want = {}


def _case(name):
    V, blank, S, shapes = _CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    cols = np.array([v for v in range(V) if v != blank])
    labels = [cols[rng.integers(0, len(cols), size=U)].tolist() for _, U, _ in shapes]
    if name == "ragged":
        labels[1] = [1, 1, 3, 1, 1, 1, 4, 4, 1]      # repeated labels
    zs = [(2.0 * rng.standard_normal((T, S, V))).astype(np.float32) for T, _, _ in shapes]
    bands = [_band(kind, T, U, S, rng) for T, U, kind in shapes]
    return zs, bands, labels, blank, ([0.5, 2.0, 0.125, 1.75] if name == "ragged" else None)


def _check(name, zs, bands, labels, blank, weights=None, status=None):
    """One call: loss, gradient, status against the restatement, zero rows outside the lattice, a second call bit-identical."""
    frames, logits, begin = [z.shape[0] for z in zs], _poisoned4(zs), _begin(bands)
    out = [transducer.pruned_loss_and_grad(logits, begin, frames, labels, blank, weights) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out)) and out[0][1].shape == logits.shape
    loss, grad, st = [o.cpu().numpy() for o in out[0]]
    assert st.tolist() == (status or [0] * len(zs))
    for n, lab in enumerate(labels):
        if st[n]:
            assert loss[n] == 0.0 and not grad[n].any()
            continue
        w = 1.0 if weights is None else float(np.float32(weights[n]))
        if (name, n) not in _want:
            _want[name, n] = P.pruned_loss_and_grad(zs[n], bands[n], lab, blank)
        want_loss, want = _want[name, n]
        err = abs(loss[n] - want_loss), np.abs(grad[n, :frames[n]] - w * want).max()
        print("%s utt %d: loss %.6f want %.6f (err %.3g) grad err %.3g" % (name, n, loss[n], want_loss, err[0], err[1]))
        assert err[0] <= 1e-3 * abs(want_loss) + 1e-4 and err[1] <= 1e-4 and not grad[n, frames[n]:].any()
    return loss, grad, st


@pytest.mark.parametrize("name", list(_CASES))
def test_pruned_loss_and_gradient_equal_the_restatement(name):
    zs, bands, labels, blank, w = _case(name)
    loss, grad, _ = _check(name, zs, bands, labels, blank, w)
    if name == "ragged":      # an utterance alone is bit-identical to its rows in the batch
        for n in range(4):
            l1, g1, _ = _check("ragged%d" % n, [zs[n]], [bands[n]], [labels[n]], blank, [w[n]])
            assert l1[0].tobytes() == loss[n].tobytes() and np.array_equal(g1[0].view(np.int32), grad[n, :zs[n].shape[0]].view(np.int32))


@pytest.mark.parametrize("bad", ["first", "step_S", "decreasing", "short", "inf"])
def test_a_bad_band_or_logit_is_a_status_and_leaves_the_neighbours_alone(bad):
    zs, bands, labels, blank, _ = _case("ragged")
    zs, bands, labels = [z.copy() for z in zs[:3]], [b.copy() for b in bands[:3]], labels[:3]
    if bad == "first":
        bands[1][0] = 1
    elif bad == "step_S":
        bands[1][:] = 5
        bands[1][0] = 0
    elif bad == "decreasing":
        bands[1][:3] = [0, 1, 0]
    elif bad == "short":
        bands[1][:] = 0
    else:
        zs[1][0, 0, 3] = np.inf
    loss, grad, _ = _check("bad", zs, bands, labels, blank, status=[0, 3 if bad == "inf" else transducer.TRANSDUCER_RANGES, 0])
    loss2, grad2, _ = _check("bad2", zs[::2], bands[::2], labels[::2], blank)
    for a, b in ((0, 0), (2, 1)):
        assert loss[a].tobytes() == loss2[b].tobytes() and np.array_equal(grad[a].view(np.int32), grad2[b, :grad.shape[1]].view(np.int32))


def test_workspace_has_no_term_in_V():
    small, large = [_lib.lib().pk2_transducer_pruned_workspace_bytes(3, 130, 5, V) for V in (43, 5768)]
    assert 0 < small == large


@pytest.mark.parametrize("shapes,S", [([(1, 0)], 2), ([(4, 3)], 2), ([(6, 2)], 5), ([(65, 40)], 5), ([(40, 3)], 32),
                                      ([(21, 2), (76, 9), (80, 10), (22, 2)], 5)])
def test_ranges_from_the_first_stage(shapes, S):
    rng = np.random.default_rng(S + len(shapes))
    V, blank = 11, 4
    cols = np.array([v for v in range(V) if v != blank])
    labels = [cols[rng.integers(0, len(cols), size=U)].tolist() for _, U in shapes]
    ams, lms = [[(2.0 * rng.standard_normal((r + k, V))).astype(np.float32) for r in rows] for k, rows in ((0, [T for T, _ in shapes]), (1, [U for _, U in shapes]))]
    am, lm, frames = _poisoned(ams, V), _poisoned(lms, V), [T for T, _ in shapes]
    plain = transducer.transducer_loss_and_grad(am, lm, frames, labels, blank)
    out = [transducer.loss_grad_and_ranges(am, lm, frames, labels, S, blank) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out)) and all(torch.equal(a, b) for a, b in zip(plain, out[0]))
    begin, gamma = out[0][4].cpu().numpy(), out[0][5].cpu().numpy()
    assert begin.dtype == np.int32 and begin.shape == am.shape[:2] and gamma.shape == am.shape[:2] + (max(U for _, U in shapes) + 1,)
    for n, (T, U) in enumerate(shapes):
        logp, _, py, px, alpha, beta = R.lattice(ams[n], lms[n], labels[n], blank)
        want = np.exp(alpha[:T, :U + 1] + py + beta[1:, :U + 1] - logp) + np.exp(alpha[:T, :U + 1] + px + beta[:T, 1:] - logp)
        assert np.abs(gamma[n, :T, :U + 1] - want).max() <= 1e-4 and not gamma[n, T:].any() and not gamma[n, :, U + 1:].any()
        assert begin[n, :T].tolist() == P.ranges(gamma[n], T, U, S).tolist() and not begin[n, T:].any()


@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_pruned_loss_under_autograd(reduction):
    zs, bands, labels, blank, _ = _case("ragged")
    frames, logits = [z.shape[0] for z in zs], _poisoned4(zs).clone().requires_grad_()
    out = ops.PrunedTransducerLoss(blank, reduction)(logits, _begin(bands), frames, labels)
    assert out.grad_fn.per_sequence.dtype == torch.float64 and out.grad_fn.status.tolist() == [0] * 4
    (out * 0.5).sum().backward()
    w = [{"sum": 1.0, "none": 1.0, "mean": 1.0 / (4 * max(len(lab), 1))}[reduction] for lab in labels]
    want = [P.pruned_loss_and_grad(z, b, lab, blank, 0.5 * wn) for z, b, lab, wn in zip(zs, bands, labels, w)]
    losses = np.array([wn * x[0] for wn, x in zip(w, want)])
    got, want_out = out.detach().cpu().numpy(), (losses if reduction == "none" else losses.sum())
    assert (np.abs(got - want_out) <= 1e-3 * np.abs(want_out) + 1e-4).all()
    for n, (_, g) in enumerate(want):
        assert np.abs(logits.grad[n, :frames[n]].cpu().numpy() - g).max() <= 1e-4


def test_transducer_loss_with_a_prune_range_returns_the_functions_begin():
    rng = np.random.default_rng(5)
    ams, lms = [(2.0 * rng.standard_normal((T, 9))).astype(np.float32) for T in (30, 17)], [(2.0 * rng.standard_normal((U + 1, 9))).astype(np.float32) for U in (12, 4)]
    labels, am, lm = [rng.integers(1, 9, size=U).tolist() for U in (12, 4)], _poisoned(ams, 9).clone().requires_grad_(), _poisoned(lms, 9).clone().requires_grad_()
    loss, begin = ops.TransducerLoss(0, "sum", prune_range=5)(am, lm, [30, 17], labels)
    want = transducer.loss_grad_and_ranges(am, lm, [30, 17], labels, 5)
    assert torch.equal(begin, want[4]) and not begin.requires_grad and loss.requires_grad
    loss.backward()
    assert torch.equal(am.grad, want[1]) and torch.equal(lm.grad, want[2])
    assert torch.equal(loss.detach(), ops.TransducerLoss(0, "sum")(am, lm, [30, 17], labels).detach())


@pytest.mark.parametrize("J", [1, 5, 512])
@pytest.mark.parametrize("tanh", [True, False])
def test_join_and_its_gradients_equal_the_restatement(J, tanh):
    """The bound: four times the error of torch's own float32 tanh(enc + pred) and autograd sums on the CPU against the same
    float64 restatement (the device's tanhf and its order of summation need not be torch's)."""
    _, _, S, shapes = _CASES["ragged"]
    rng = np.random.default_rng(J)
    bands, frames, counts = [_band(kind, T, U, S, rng) for T, U, kind in shapes], [T for T, _, _ in shapes], [U for _, U, _ in shapes]
    encs, preds = [[rng.standard_normal((r + k, J)).astype(np.float32) for r in rows] for k, rows in ((0, frames), (1, counts))]
    dhs = [rng.standard_normal((T, S, J)).astype(np.float32) for T in frames]
    enc, pred, begin = _poisoned(encs, J), _poisoned(preds, J), _begin(bands)
    if J == 512:      # dense and 16-byte aligned: the forward's 16-byte path (the views above: its scalar path)
        enc, pred = enc.clone(), pred.clone()
    enc.requires_grad_(), pred.requires_grad_()
    dh = torch.zeros((4, enc.shape[1], S, J), device="cuda")
    for n, x in enumerate(dhs):
        dh[n, :frames[n]] = torch.from_numpy(x)
    res = []
    for _ in range(2):
        enc.grad = pred.grad = None
        h = ops.PrunedJoin.apply(enc, pred, begin, frames, counts, S, tanh)
        h.backward(dh)
        res.append((h.detach(), enc.grad, pred.grad))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and res[0][0].shape == (4, enc.shape[1], S, J)
    got, err, ref = [x.cpu().numpy() for x in res[0]], np.zeros(3), np.zeros(3)
    for n, (T, U) in enumerate(zip(frames, counts)):
        want = P.join(encs[n], preds[n], bands[n], T, U, S, tanh, dhs[n])
        e, p = torch.from_numpy(encs[n]).requires_grad_(), torch.from_numpy(preds[n]).requires_grad_()
        u = torch.from_numpy(bands[n])[:, None] + torch.arange(S)
        x = e[:, None, :] + p[u.clamp(max=U)]
        y = (torch.tanh(x) if tanh else x) * (u <= U)[:, :, None]
        y.backward(torch.from_numpy(dhs[n]))
        cpu = (y.detach().numpy(), e.grad.numpy(), p.grad.numpy())
        for i in range(3):
            err[i] = max(err[i], np.abs(got[i][n, :want[i].shape[0]] - want[i]).max())
            ref[i] = max(ref[i], np.abs(cpu[i] - want[i]).max())
        assert not got[0][n, T:].any() and not got[1][n, T:].any() and not got[2][n, U + 1:].any()
    print("join J %d tanh %d: device errors %s, torch CPU float32 errors %s" % (J, tanh, err, ref))
    assert (err <= 4 * ref).all()
