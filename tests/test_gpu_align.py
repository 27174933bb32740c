"""The device Viterbi of the forced aligner (csrc/align_viterbi.hip) against the float32 emulation of its specified
arithmetic (tests/test_align_graph.py: emulate_viterbi) -- costs, transition-ids and statuses bit for bit -- and against a
float64 Viterbi on planted-path data; the beam and retry_beam; MappedAligner.align / align_batch."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import chain, synth

import graph_cases as GC
from graph_cases import planted as _planted
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


# ---------------------------------------------------------------- graphs beyond 1024 states (tests/graph_cases.py)
def _nan_buffer(ll_list):
    """The utterances' log-likelihoods inside a NaN-filled buffer: row stride PDFS + 9, padded frames NaN."""
    N, Tmax = len(ll_list), max(ll.shape[0] for ll in ll_list)
    big = torch.full((N, Tmax + 3, PDFS + 9), float("nan"), dtype=torch.float32, device="cuda")
    x = big[:, :Tmax, :PDFS]
    for n, ll in enumerate(ll_list):
        x[n, :ll.shape[0]] = torch.from_numpy(ll).cuda()
    return x


def _run(graphs, x, beam):
    return [t.cpu().numpy() for t in chain.align_viterbi(graphs, x, GC.ASCALE, beam)]


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2], b[2])


def _check_row(got, n, T, ref):
    """Row n of a launch against an emulation result: status, transition-ids and the three costs bit for bit."""
    ali, costs, status = got
    st, tids, tot, gc, ac = ref
    assert status[n] == st, (n, status[n], st)
    assert (ali[n, T:] == 0).all()
    if st == 0:
        assert np.array_equal(ali[n, :T], tids), (n, int((ali[n, :T] != tids).sum()))
        assert np.array_equal(costs[n].view(np.int32), np.asarray([tot, gc, ac], np.float32).view(np.int32)), (n, costs[n], tot, gc, ac)
    else:
        assert (ali[n] == 0).all() and np.isinf(costs[n]).all()


def _ladder_references(k):
    """Both emulations of rung k, with what the binding beam must have done on the CPU."""
    wide, _ = GC.viterbi_reference(k, 1e30)
    tight, trace = GC.viterbi_reference(k, GC.BINDING_BEAM[k])
    assert wide[0] == 0 and tight[0] == 0 and trace["pruned"] > 0
    assert GC.differs(wide, tight), "rung %d: the beam %g does not change the alignment" % (k, GC.BINDING_BEAM[k])
    return {1e30: wide, GC.BINDING_BEAM[k]: tight}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ladder_bit_exact(monkeypatch, k):
    """One utterance per rung, T = minimum + 50: 4, 8 and 16 states per thread; LDS below 64 KiB, above it (the opt-in
    attribute), and global memory chosen by size.  Rungs 1 and 2 again with the graph forced out of LDS."""
    monkeypatch.delenv("PK2_ALIGN_LDS", raising=False)
    words, T = GC.rung(k)
    model, lexicon = GC.triphone()
    graphs = chain.AlignmentGraphs(model, lexicon, [words], [T])
    assert graphs.status == [0], graphs.errors
    S, A = graphs.num_states[0], graphs.num_arcs[0]
    GC.assert_rung(k, S)
    lds = GC.viterbi_lds(S, A)
    if k == 1:
        assert lds <= GC.LDS_OPT_IN and graphs.uses_lds()
    elif k == 2:
        assert GC.LDS_OPT_IN < lds <= GC.LDS_LIMIT and graphs.uses_lds()
    else:
        assert lds > GC.LDS_LIMIT and not graphs.uses_lds()
    print("rung %d: S %d A %d T %d, %d states per thread, LDS %d bytes -> %s" % (
        k, S, A, T, GC.states_per_thread(S), lds, "LDS" if graphs.uses_lds() else "global"))
    x = _nan_buffer([GC.rung_loglikes(k)])
    for beam, ref in _ladder_references(k).items():
        got = _run(graphs, x, beam)
        _check_row(got, 0, T, ref)
        if k < 3:
            monkeypatch.setenv("PK2_ALIGN_LDS", "0")
            assert not graphs.uses_lds()
            assert _same_bits(_run(graphs, x, beam), got)
            monkeypatch.delenv("PK2_ALIGN_LDS")


def test_widest_route_in_a_mixed_batch(monkeypatch):
    """Rung 4 (32 states per thread, global memory by size) in one launch with a two-word utterance, a one-word utterance
    at its minimum length and one without a path: everything runs on the route of the largest graph."""
    monkeypatch.delenv("PK2_ALIGN_LDS", raising=False)
    model, lexicon = GC.triphone()
    words, T = GC.rung(4)
    one = [4]
    texts = [words, [2, 4], one, [5, 5, 5, 5]]
    frames = [T, 40, GC.min_frames(one, hi=64), 14]
    graphs = chain.AlignmentGraphs(model, lexicon, texts, frames)
    assert graphs.status == [0, 0, 0, chain.ALIGN_NO_PATH], graphs.errors
    S, A = graphs.num_states[0], graphs.num_arcs[0]
    GC.assert_rung(4, S)
    assert S > 8192 and GC.states_per_thread(max(graphs.num_states)) == 32
    assert GC.viterbi_lds(S, A) > GC.LDS_LIMIT and not graphs.uses_lds()
    print("rung 4: S %d A %d T %d, 32 states per thread, LDS %d bytes -> global; neighbours S %s T %s" % (
        S, A, T, GC.viterbi_lds(S, A), graphs.num_states[1:], frames[1:]))
    rng = np.random.default_rng(31)
    lls = [GC.rung_loglikes(4)] + [(3.0 * rng.standard_normal((t, PDFS))).astype(np.float32) for t in frames[1:]]
    x = _nan_buffer(lls)
    small = chain.AlignmentGraphs(model, lexicon, texts[1:3], frames[1:3])
    assert small.status == [0, 0] and GC.states_per_thread(max(small.num_states)) == 1 and small.uses_lds()
    xs = _nan_buffer(lls[1:3])
    for beam, ref in _ladder_references(4).items():
        got = _run(graphs, x, beam)
        _check_row(got, 0, T, ref)
        for n in (1, 2):
            _check_row(got, n, frames[n], emulate_viterbi(graphs.export(n), lls[n], GC.ASCALE, beam))
        assert got[2][3] == chain.ALIGN_NO_PATH and (got[0][3] == 0).all() and (got[1][3] == np.inf).all()
        assert (got[2][:3] == 0).all()
        # the small utterances alone run with one state per thread in LDS: the arithmetic does not depend on the route
        alone = _run(small, xs, beam)
        for n in (1, 2):
            assert np.array_equal(alone[0][n - 1, :frames[n]], got[0][n, :frames[n]])
            assert np.array_equal(alone[1][n - 1].view(np.int32), got[1][n].view(np.int32)) and alone[2][n - 1] == got[2][n]


def test_ties_bit_exact():
    """Only the lexicon's costs and all-zero log-likelihoods on more than 1024 states: exact ties at almost every state,
    and between two final states; strict < keeps the first arc in stored order, the lowest final state wins."""
    graphs, T, beams = GC.ties_case()
    S = graphs.num_states[0]
    assert S > 1024 and graphs.status == [0]
    ll = np.zeros((T, PDFS), np.float32)
    x = _nan_buffer([ll])
    for beam in beams:
        ref, trace = GC.ties_reference(beam)
        assert ref[0] == 0 and trace["arc_ties"] > 0 and trace["final_ties"] >= 2
        _check_row(_run(graphs, x, beam), 0, T, ref)
