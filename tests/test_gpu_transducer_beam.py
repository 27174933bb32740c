"""Transducer beam search on the device (csrc/transducer_beam.hip) against the float64 oracles: tests/
transducer_ref.py for the exact posterior of every label sequence (1) and the dict restatement tests/transducer_beam_ref.py
for the pruned search (2).  Scores are held to the chain path's tolerance, 1e-3 |want| + 1e-4.  The surviving set is only
comparable where float32 rounding cannot flip a cut, so every case of (2) first asserts, on the restatement alone, that its
smallest gap (beam cuts on scores, token cuts on logits) is at least T (R + 1) E: the emissions on a path times the error E
of one emission's lp = (z - M) - log Z on BOTH compared values, in unit roundoffs u = 2^-24:
    dz  additive: A u, the one rounding of am + table, A = max |z|.
        joiner:   W1 (Ah + 2) u + (J + 2) W1 u.  h = tanhf(enc + pred): the sum's rounding Ah u (Ah = max |enc + pred|) passes
                  tanh' <= 1, tanhf itself is good to 2 ulp of |h| <= 1; either reaches z through W1 = max_v (sum_j |w_out[v, j]|
                  + |b_out[v]|); then a product of J terms and the bias, in any order: (J + 2) u sum |h w| <= (J + 2) u W1.
    lp  2 dz (z, and Z's terms) + u (2 S + V / 64 + 2 ln V + 10): S = max (M - z) is the rounding of z - M and the argument
        error of exp, exp and log are good to 2 ulp, a lane sums V / 64 terms and the wave 6 more.
    E = 2 (2 dz + u (2 S + V / 64 + 2 ln V + 10)).
The seeds below were chosen on the CPU so that every utterance of every case meets it."""
import itertools
import math

import numpy as np
import pytest
import torch

from pykaldi2_amd import transducer

import transducer_beam_ref as B
import transducer_ref as R

gpu = pytest.mark.gpu

# name: (V, frames, beam, top_tokens, max_symbols, blank, J (0: additive), table / pred / w_out dense instead of poisoned views, seed)
CASES = {
    "blank_first": (7, [6, 4], 5, 4, 2, 0, 0, False, 1),               # K < V - 1: the token cut bites
    "blank_middle": (7, [6, 4], 5, 4, 2, 3, 0, False, 1),
    "blank_last": (7, [6, 4], 5, 4, 2, 6, 0, False, 1),
    "T1_T0": (5, [1, 0, 3], 4, 4, 2, 0, 0, False, 1),
    "beam1_R1": (8, [8, 5], 1, 7, 1, 0, 0, False, 1),
    "beam32_R3": (12, [6, 5], 32, 8, 3, 0, 0, False, 1),               # the full tile, 256 candidates
    "ragged": (23, [40, 7, 33, 19], 4, 4, 2, 7, 0, False, 1),
    "J2": (7, [5, 3], 4, 3, 2, 0, 2, False, 1),                        # one MFMA k step
    "J33": (9, [5, 3], 4, 4, 2, 8, 33, False, 1),                      # odd, padded
    "J64_V33": (33, [5, 4], 8, 6, 2, 0, 64, True, 17),                 # 16-byte loads; one column past a tile
    "J512_V1031": (1031, [3, 2], 3, 2, 1, 1030, 512, True, 4),         # neither w_out nor the logits fit in LDS
    "V5": (5, [5, 3], 32, 4, 2, 0, 16, False, 1),                      # less than one column tile, the full row tile
    "V97": (97, [5, 3], 5, 8, 3, 0, 24, False, 2),
    "J64_strided": (12, [5, 4], 4, 4, 2, 0, 64, False, 6),             # J % 8 == 0 but rows of 73 floats: scalar loads
}
_want = {}


def _case(name):
    """Per utterance the float32 operands: additive (am [T, V], table) or joiner (enc [T, J], pred, w_out, b_out)."""
    V, frames, beam, K, Rm, blank, J, strided, seed = CASES[name]
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)
    if J == 0:
        shared = (f32(rng.standard_normal((V, V))),)
    else:
        shared = (f32(rng.standard_normal((V, J))), f32(3.0 / math.sqrt(J) * rng.standard_normal((V, J))), f32(0.5 * rng.standard_normal(V)))
    xs = [f32((2.0 if J == 0 else 1.0) * rng.standard_normal((T, J or V))) for T in frames]
    return xs, shared, dict(blank=blank, beam=beam, top_tokens=K, max_symbols=Rm)


def _bound(name, x, shared):
    V, _, _, _, Rm, _, J, _, _ = CASES[name]
    u, z = 2.0 ** -24, (B.joiner if J else B.additive)(x, *shared)
    zs = np.stack([z(t, p) for t in range(len(x)) for p in range(V)])
    if J:
        W1 = (np.abs(shared[1]).sum(1) + np.abs(shared[2])).max()
        dz = W1 * (np.abs(x[:, None, :] + shared[0][None]).max() + 2) * u + (J + 2) * W1 * u
    else:
        dz = np.abs(zs).max() * u
    S = (zs.max(1, keepdims=True) - zs).max()
    return len(x) * (Rm + 1) * 2 * (2 * dz + u * (2 * S + V / 64 + 2 * math.log(V) + 10))


def _reference(name):
    """The restatement's N-best of every utterance of the case, after the precondition on the reference alone."""
    if name not in _want:
        xs, shared, kw = _case(name)
        z = B.joiner if CASES[name][6] else B.additive
        _want[name] = [B.beam_search(z(x, *shared), len(x), **kw) for x in xs]
        for x, (_, gap) in zip(xs, _want[name]):
            print("%s T %d: gap %.3g (bound %.3g)" % (name, len(x), gap, _bound(name, x, shared) if len(x) else 0.0))
            assert len(x) == 0 or gap >= _bound(name, x, shared)
    return [w[0] for w in _want[name]]


def _poisoned(a):
    """A float32 array as a view into a larger NaN-filled device buffer (as tests/test_gpu_ctc_beam.py does)."""
    big = torch.full([s + 3 for s in a.shape[:-1]] + [a.shape[-1] + 9], float("nan"), dtype=torch.float32, device="cuda")
    view = big[tuple(slice(0, s) for s in a.shape)]
    view.copy_(torch.from_numpy(a))
    return view


def _inputs(name, time_major):
    """(x [N, T, D] or [T, N, D], poisoned, NaN in the rows past a length; table or pred; the keyword arguments)."""
    xs, shared, kw = _case(name)
    full = np.full((len(xs), max(len(x) for x in xs), xs[0].shape[1]), np.nan, np.float32)
    for n, a in enumerate(xs):
        full[n, :len(a)] = a
    x = _poisoned(np.ascontiguousarray(full.transpose(1, 0, 2)) if time_major else full)
    dev = [torch.from_numpy(a).cuda() if (CASES[name][7] or a.ndim == 1) else _poisoned(a) for a in shared]
    if len(dev) == 3:
        kw = dict(kw, joiner=(dev[1], dev[2]))
    return x, dev[0], kw


def _nbest(out, n):
    tok, lens, sc = [o[n].cpu().numpy() for o in out[:3]]
    assert (tok[np.arange(tok.shape[1])[None, :] >= np.maximum(lens, 0)[:, None]] == -1).all()
    return [(tuple(tok[r, :lens[r]].tolist()), float(sc[r])) for r in range(len(lens)) if lens[r] >= 0]


def _compare(got, want, what):
    assert [s for _, s in got] == sorted((s for _, s in got), reverse=True), what
    assert len(got) == len(want) and set(dict(got)) == set(dict(want)), (what, set(dict(got)) ^ set(dict(want)))
    for l, s in got:
        assert abs(s - dict(want)[l]) <= 1e-3 * abs(dict(want)[l]) + 1e-4, (what, l, s, dict(want)[l])
    assert got[0][0] == want[0][0], what


@gpu
@pytest.mark.parametrize("V,T,Rm,beam", [(3, 2, 2, 32), (2, 5, 3, 16)])
def test_every_sequence_has_its_exact_posterior(V, T, Rm, beam):
    """beam >= the number of reachable sequences and every token kept: nothing is pruned, so the N-best is every label sequence
    of at most T R labels, and one of at most R labels (no alignment needs more than R on a frame) scores minus its loss."""
    rng = np.random.default_rng(V)
    am, table = (2.0 * rng.standard_normal((T, V))).astype(np.float32), rng.standard_normal((V, V)).astype(np.float32)
    blank = V - 1
    out = transducer.beam_search_raw(_poisoned(am[None]), [T], _poisoned(table), blank=blank, beam=beam, top_tokens=V - 1, max_symbols=Rm)
    got = _nbest(out, 0)
    seqs = [l for L in range(T * Rm + 1) for l in itertools.product(range(V - 1), repeat=L)]
    assert out[3].tolist() == [0] and sorted(l for l, _ in got) == sorted(seqs)
    ref = dict(B.beam_search(B.additive(am, table), T, blank, beam, V - 1, Rm)[0])
    for l, s in got:
        want = -R.loss_and_grad(am, table[[blank] + list(l)], list(l), blank)[0] if len(l) <= Rm else ref[l]
        assert abs(s - want) <= 1e-3 * abs(want) + 1e-4, (l, s, want)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_restatement(name):
    want = _reference(name)
    frames = CASES[name][1]
    for time_major in (False, True):
        x, rows, kw = _inputs(name, time_major)
        out, again = [transducer.beam_search_raw(x, frames, rows, time_major=time_major, **kw) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(out, again)) and out[3].tolist() == [0] * len(frames)
        for n in range(len(frames)):
            _compare(_nbest(out, n), want[n], (name, n, time_major))
        if name == "ragged" and not time_major:      # an utterance alone, at the same addresses: bit-identical to its part of the batch
            for n in range(len(frames)):
                alone = transducer.beam_search_raw(x[n:n + 1], frames[n:n + 1], rows, **kw)
                assert all(torch.equal(a[0], b[n]) for a, b in zip(alone, out))
            best = transducer.beam_search(x, frames, rows, nbest=2, **kw)      # the list form: one copy to the host
            assert [[(tuple(l), s) for l, s in h] for h in best] == [_nbest(out, n)[:2] for n in range(len(frames))]


@pytest.mark.parametrize("kw", [dict(beam=0), dict(beam=33), dict(top_tokens=33), dict(max_symbols=0), dict(J=513), dict(table=(5, 4)),
                                dict(J=8, pred=(5, 7)), dict(J=8, w=(4, 8)), dict(J=8, b=(4,)), dict(lengths=[4])])
def test_host_errors(kw):
    """ValueError before anything is launched (no device needed): the limits, a table that is not [V, V], pred / w_out / b_out
    that do not go with enc, a length beyond T."""
    kw = dict(kw)
    J, lengths = kw.pop("J", 0), kw.pop("lengths", [3])
    rows = torch.zeros(kw.pop("pred", (5, J)) if J else kw.pop("table", (5, 5)))
    if J:
        kw["joiner"] = (torch.zeros(kw.pop("w", (5, J))), torch.zeros(kw.pop("b", (5,))))
    with pytest.raises(ValueError):
        transducer.beam_search_raw(torch.zeros(1, 3, J or 5), lengths, rows, **kw)
