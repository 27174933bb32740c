"""CTC prefix beam search on the device (csrc/ctc_beam.hip) against the float64 oracles: tests/ctc_ref.py for
the exact posterior of every prefix (A) and the dict restatement tests/ctc_beam_ref.py for the pruned search (B).  Scores
are held to the chain path's tolerance, 1e-3 |want| + 1e-4.  The set of surviving prefixes is only comparable where rounding
cannot flip a prune, so every case of B first asserts, on the reference alone, that the smallest relative gap between the
last kept and the first dropped candidate is at least 4 T 2^-23 (two float32 ulps per emission over T frames on each of the
two values); the seeds below were chosen on the CPU for that."""
import itertools

import numpy as np
import pytest
import torch

from pykaldi2_amd import ctc, ngram

import ctc_beam_ref as B
import ctc_ref as R

gpu = pytest.mark.gpu

# name: (P, frames, beam, top_tokens, blank, blank bias, seed, LM, merges wanted)
CASES = {
    "T1_T0": (5, [1, 0, 3], 4, 4, 0, 0.0, 1, None, False),
    "beam1": (8, [20, 12], 1, 7, 0, 0.0, 1, None, False),
    "beam64": (40, [40, 37], 64, 8, 0, 3.0, 3, None, True),            # slots fill exactly one wave
    "beam65": (40, [40, 37], 65, 8, 0, 3.0, 2, None, True),            # and cross it
    "limit": (40, [30, 26], 128, 32, 0, 3.0, 2, None, True),           # 4224 candidates
    "P61_K4": (61, [30, 17], 8, 4, 60, 0.0, 1, None, False),           # token pruning bites; rows of no whole float4s
    "P5768": (5768, [25, 11], 16, 32, 5767, 0.0, 1, None, False),      # the wide-row top-K
    "blank_first": (7, [14, 9], 8, 6, 0, 3.0, 1, None, True),
    "blank_middle": (7, [14, 9], 8, 6, 3, 3.0, 1, None, True),
    "blank_last": (7, [14, 9], 8, 6, 6, 3.0, 1, None, True),
    "T400": (601, [400, 390], 4, 8, 0, 0.0, 3, None, False),           # the best total ends near 2^-1280: not a float64 unscaled
    "ragged": (23, [40, 7, 33, 19], 8, 8, 7, 3.0, 1, None, True),      # (P + 9 columns of padding: every row 16-byte aligned)
    "trigram_eos": (7, [16, 11], 12, 6, 2, 3.0, 1, "tri", True),
    "trigram_no_eos": (7, [16, 11], 12, 6, 2, 3.0, 1, "tri_no_eos", True),
    "unigram": (7, [16, 11], 12, 6, 2, 3.0, 1, "uni", True),
}
_want, _lms = {}, {}


def _poisoned(xs, P, time_major):
    """The utterances' logits inside a larger NaN-filled buffer, as [N, T, P] or [T, N, P] (as tests/test_gpu_ctc.py does)."""
    N, Tmax = len(xs), max(x.shape[0] for x in xs)
    big = torch.full((Tmax + 3, N, P + 9) if time_major else (N, Tmax + 3, P + 9), float("nan"), dtype=torch.float32, device="cuda")
    view = big[:Tmax, :, :P] if time_major else big[:, :Tmax, :P]
    for n, x in enumerate(xs):
        (view[:x.shape[0], n] if time_major else view[n, :x.shape[0]]).copy_(torch.from_numpy(x))
    return view


def _lm(kind):
    """A seeded backoff LM over the word ids 1..6 (<s> 7, </s> 8): unigrams, ~half of the bigrams, ~a third of their trigrams."""
    order = 1 if kind == "uni" else 3
    if order not in _lms:
        rng = np.random.default_rng(11)
        words = list(range(1, 9))
        grams = {(w,): (-rng.uniform(0.3, 2.0), -rng.uniform(0.0, 0.5)) for w in words}
        for k in (2, 3)[:order - 1]:
            for g in [g + (w,) for g in list(grams) if len(g) == k - 1 and g[-1] != 8 for w in words[:6] + [8]]:
                if rng.random() < (0.5 if k == 2 else 0.35):
                    grams[g] = (-rng.uniform(0.1, 2.0), -rng.uniform(0.0, 0.5) if k < order else None)
        _lms[order] = ngram.NgramLM.from_ngrams(grams, 7, 8, order)
    return _lms[order]


def _case(name):
    P, frames, beam, K, blank, bias, seed, lm, merges = CASES[name]
    rng = np.random.default_rng(seed)
    xs = [(2.0 * rng.standard_normal((T, P))).astype(np.float32) for T in frames]
    for x in xs:
        x[:, blank] += np.float32(bias)
    kw = dict(blank=blank, beam=beam, top_tokens=K)
    if lm:
        ids = np.zeros(P, np.int64)
        ids[[c for c in range(P) if c != blank]] = [4, 1, 6, 2, 5, 3]
        kw.update(lm=_lm(lm), lm_weight=0.7, insertion_bonus=0.3, lm_ids=ids, lm_eos=lm != "tri_no_eos")
    return xs, kw, merges


def _reference(name):
    """The restatement's N-best of every utterance of the case, after the preconditions on the reference alone."""
    if name not in _want:
        xs, kw, merges = _case(name)
        _want[name] = [B.beam_search(x, **kw) for x in xs]
        for x, (_, gap, m) in zip(xs, _want[name]):
            print("%s T %d: gap %.3g (bound %.3g) merges %d" % (name, len(x), gap, 4 * len(x) * 2.0 ** -23, m))
            assert gap >= 4 * len(x) * 2.0 ** -23
        assert not merges or sum(w[2] for w in _want[name]) > 0
    return [w[0] for w in _want[name]]


def _nbest(out, n):
    tok, lens, sc = [o[n].cpu().numpy() for o in out[:3]]
    return [(tuple(tok[r, :lens[r]].tolist()), float(sc[r])) for r in range(len(lens)) if lens[r] >= 0]


def _compare(got, want, what):
    assert [s for _, s in got] == sorted((s for _, s in got), reverse=True), what
    assert len(got) == len(want) and set(dict(got)) == set(dict(want)), (what, set(dict(got)) ^ set(dict(want)))
    for l, s in got:
        assert abs(s - dict(want)[l]) <= 1e-3 * abs(dict(want)[l]) + 1e-4, (what, l, s, dict(want)[l])
    assert got[0][0] == want[0][0], what


@gpu
@pytest.mark.parametrize("P,T,beam,blank", [(3, 4, 32, 1), (2, 6, 8, 0)])
def test_every_prefix_has_its_exact_posterior(P, T, beam, blank):
    """beam >= the number of reachable prefixes and every token kept: nothing is pruned, so the N-best is every label
    sequence with an alignment and each score is minus its CTC loss (the pb / pnb split, repeats, the merge)."""
    x = (2.0 * np.random.default_rng(P).standard_normal((T, P))).astype(np.float32)
    x[:, blank] += np.float32(3.0)
    out = ctc.beam_search_raw(_poisoned([x], P, False), [T], blank=blank, beam=beam, top_tokens=P - 1)
    got = _nbest(out, 0)
    cols = [c for c in range(P) if c != blank]
    seqs = [l for L in range(T + 1) for l in itertools.product(cols, repeat=L) if L + sum(a == b for a, b in zip(l, l[1:])) <= T]
    assert out[3].tolist() == [0] and sorted(l for l, _ in got) == sorted(seqs)
    for l, s in got:
        want = -R.loss_and_grad(x, list(l), blank)[0]
        assert abs(s - want) <= 1e-3 * abs(want) + 1e-4, (l, s, want)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_restatement(name):
    xs, kw, _ = _case(name)
    want = _reference(name)
    for time_major in (False, True):
        x = _poisoned(xs, xs[0].shape[1], time_major)
        frames = [len(a) for a in xs]
        out, again = [ctc.beam_search_raw(x, frames, time_major=time_major, **kw) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(out, again)) and out[3].tolist() == [0] * len(xs)
        for n in range(len(xs)):
            _compare(_nbest(out, n), want[n], (name, n, time_major))
        if name == "ragged" and not time_major:      # an utterance alone, at the same addresses: bit-identical to its part of the batch
            for n in range(len(xs)):
                alone = ctc.beam_search_raw(x[n:n + 1], frames[n:n + 1], **kw)
                assert all(torch.equal(a[0], b[n]) for a, b in zip(alone, out))
            best = ctc.beam_search(x, frames, nbest=2, **kw)      # the list form: one copy to the host
            assert [[(tuple(l), s) for l, s in h] for h in best] == [_nbest(out, n)[:2] for n in range(len(xs))]


@pytest.mark.parametrize("kw", [dict(beam=0), dict(beam=129), dict(top_tokens=33), dict(lm="tri"), dict(lm="tri", lm_ids=[1, 2, 3])])
def test_host_errors(kw):
    """ValueError before anything is launched (no device needed): the limits, a column without a unigram (the identity maps
    column 0 to word 0, which the LM does not have), an lm_ids of the wrong length."""
    if "lm" in kw:
        kw = dict(kw, lm=_lm(kw["lm"]), blank=4)
    with pytest.raises(ValueError):
        ctc.beam_search_raw(torch.zeros(1, 3, 5), [3], **kw)
