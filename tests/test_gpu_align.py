"""The device Viterbi of the forced aligner (csrc/align_viterbi.hip) against the float32 emulation of its specified
arithmetic (tests/test_align_graph.py: emulate_viterbi) -- costs, transition-ids and statuses bit for bit -- and against a
float64 Viterbi on planted-path data; the beam and retry_beam; MappedAligner.align / align_batch."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import chain, synth

from test_align_graph import PRONS, emulate_viterbi, exported_arcs, kaldi_like_lexicon, make_model, viterbi64

pytestmark = pytest.mark.gpu

PDFS = 60


def _triphone():
    tree, tm = make_model(7, 3, 1, seed=7, num_pdfs=PDFS)
    return chain.AlignModel(tree, tm, 1.0, 0.1), chain.Lexicon(kaldi_like_lexicon(PRONS), [9, 10]), tm


def _batch(rng):
    texts, frames = [], []
    for n in range(7):
        k = int(rng.integers(1, 5))
        texts.append([int(w) for w in rng.integers(1, 6, size=k)])
        frames.append(int(rng.integers(12 * k + 8, 12 * k + 60)))
    texts.append([int(w) for w in rng.integers(1, 6, size=26)])     # > 512 states: several states per lane
    frames.append(420)
    texts[2], frames[2] = [5, 5, 5, 5], 14                          # no path of 14 frames
    return texts, frames


def _check_against_emulation(graphs, ll_list, x, ascale, beam):
    ali, costs, status = (t.cpu().numpy() for t in chain.align_viterbi(graphs, x, ascale, beam))
    for n, ll in enumerate(ll_list):
        T = ll.shape[0]
        assert (ali[n, T:] == 0).all()
        if graphs.status[n] != 0:
            assert status[n] == graphs.status[n] and (ali[n] == 0).all() and np.isinf(costs[n]).all()
            continue
        st, tids, tot, gc, ac = emulate_viterbi(graphs.export(n), ll, ascale, beam)
        assert status[n] == st, n
        if st == 0:
            assert np.array_equal(ali[n, :T], tids), n
            assert np.array_equal(costs[n].view(np.int32), np.asarray([tot, gc, ac], np.float32).view(np.int32)), (n, costs[n], tot, gc, ac)
        else:
            assert (ali[n] == 0).all() and np.isinf(costs[n]).all()
    return ali, costs, status


@pytest.mark.parametrize("lds", ["1", "0"])
def test_batch_bit_exact_in_nan_buffer(monkeypatch, lds):
    monkeypatch.setenv("PK2_ALIGN_LDS", lds)
    model, lexicon, _ = _triphone()
    rng = np.random.default_rng(11)
    texts, frames = _batch(rng)
    graphs = chain.AlignmentGraphs(model, lexicon, texts, frames)
    assert graphs.status[2] == chain.ALIGN_NO_PATH and graphs.status.count(0) == 7
    assert max(graphs.num_states) > 512
    assert graphs.uses_lds() == (lds == "1")
    N, Tmax = len(texts), max(frames)
    big = torch.full((N, Tmax + 3, PDFS + 9), float("nan"), dtype=torch.float32, device="cuda")
    x = big[:, :Tmax, :PDFS]                       # row stride PDFS + 9, padded frames NaN
    ll_list = []
    for n, T in enumerate(frames):
        ll = (3.0 * rng.standard_normal((T, PDFS))).astype(np.float32)
        ll_list.append(ll)
        x[n, :T] = torch.from_numpy(ll).cuda()
    for beam in (4.0, 1e30):
        ali, costs, status = _check_against_emulation(graphs, ll_list, x, 0.1, beam)
        assert (status == 0).sum() >= 5
        again = [t.cpu().numpy() for t in chain.align_viterbi(graphs, x, 0.1, beam)]
        assert np.array_equal(again[0], ali) and np.array_equal(again[1].view(np.int32), costs.view(np.int32))
        assert np.array_equal(again[2], status)


def _planted(rng, graph, T, pdfs, peak=8.0):
    """A random path of exactly T frames through an exported graph, and log-likelihoods peaked along its pdfs."""
    S = graph["final"].shape[0]
    src, dst = graph["src"], graph["dst"]
    reach = np.zeros((T, S), bool)
    reach[0, dst[src < 0]] = True
    for t in range(1, T):
        ok = (src >= 0) & reach[t - 1, np.maximum(src, 0)]
        reach[t, dst[ok]] = True
    cand = np.flatnonzero(reach[T - 1] & np.isfinite(graph["final"]))
    s = int(rng.choice(cand))
    arcs = []
    for t in range(T - 1, -1, -1):
        ks = np.flatnonzero((dst == s) & ((src < 0) if t == 0 else ((src >= 0) & reach[t - 1, np.maximum(src, 0)])))
        k = int(rng.choice(ks))
        arcs.append(k)
        s = int(src[k])
    arcs = arcs[::-1]
    ll = rng.uniform(-1.0, 0.0, (T, pdfs)).astype(np.float32) - peak
    ll[np.arange(T), graph["pdf"][arcs]] = 0.0
    return ll, graph["tid"][arcs]


def _synthetic_aligner(beam=10.0, retry_beam=None):
    P = 60
    tree, tm = synth.alignment_model(P)
    lex = synth.lexicon_arcs(30, P, seed=5, max_phones=3)
    return chain.MappedAligner.from_models(tm, tree, lex, beam=beam, transition_scale=1.0, self_loop_scale=0.1,
                                           acoustic_scale=0.1, retry_beam=retry_beam), tm, P


def test_planted_paths_close_to_float64():
    aligner, tm, P = _synthetic_aligner()
    rng = np.random.default_rng(3)
    texts = [[int(w) for w in rng.integers(2, 31, size=k)] for k in (1, 3, 5, 2)]
    frames = [40, 90, 160, 70]
    graphs = aligner.compile(texts, frames)
    lls, planted = [], []
    for n, T in enumerate(frames):
        ll, tids = _planted(rng, graphs.export(n), T, P)
        lls.append(ll); planted.append(tids)
    x = torch.zeros(len(frames), max(frames), P, device="cuda")
    for n, ll in enumerate(lls):
        x[n, :ll.shape[0]] = torch.from_numpy(ll).cuda()
    out = aligner.align_batch(x, frames, texts)
    for n, r in enumerate(out):
        assert r is not None
        ex = graphs.export(n)
        want, want_tids = viterbi64(ex["final"].shape[0], exported_arcs(ex), ex["final"].astype(np.float64), lls[n], 0.1)
        got = -r["likelihood"]
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
        assert abs(sum(r["weight"]) - want) <= 1e-5 * abs(want)
        ok, phones = chain.split_to_phones(tm, r["alignment"])
        ok_p, planted_phones = chain.split_to_phones(tm, planted[n])
        assert ok and ok_p and [p[0] for p in phones] == [p[0] for p in planted_phones]
        assert r["alignment"] == want_tids
    # single-utterance form, text as a string
    r = aligner.align(torch.from_numpy(lls[1]), " ".join(map(str, texts[1])))
    assert r["alignment"] == out[1]["alignment"] and r["likelihood"] == out[1]["likelihood"]


def test_beam_failure_and_retry():
    aligner, tm, P = _synthetic_aligner(beam=1.0, retry_beam=10.0)
    rng = np.random.default_rng(8)
    text, T = [4, 9], 50
    graphs = aligner.compile([text], [T])
    ex = graphs.export(0)
    base, _ = _planted(rng, ex, T, P)
    # at the last frame a non-final state is far more likely than any final one: the first pdf (in a fixed order) for
    # which a beam of 1 loses every final state and a beam of 10 keeps one
    fin = np.isfinite(ex["final"])
    for pdf in np.unique(ex["pdf"][~fin[ex["dst"]]]):
        ll = base.copy()
        ll[T - 1, pdf] = 40.0
        small, wide = emulate_viterbi(ex, ll, 0.1, 1.0), emulate_viterbi(ex, ll, 0.1, 10.0)
        if small[0] == chain.ALIGN_BEAM and wide[0] == 0:
            break
    else:
        raise AssertionError("no planted beam failure found")
    x = torch.from_numpy(ll).cuda()[None]
    for beam, want in ((1.0, 1), (10.0, 0)):
        _, _, status = chain.align_viterbi(graphs, x, 0.1, beam)
        assert int(status[0]) == want
    assert aligner.align_batch(x, [T], [text]) == [None]
    r = aligner.align(x[0], text)                      # retried at retry_beam = 10
    assert np.array_equal(r["alignment"], wide[1])
    plain, _, _ = _synthetic_aligner(beam=1.0)
    with pytest.raises(RuntimeError, match="beam"):
        plain.align(x[0], text)
