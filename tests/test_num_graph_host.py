"""Alignment-free LF-MMI numerator, host side: the float64 oracle (tests/num_graph_ref.py) pinned against a brute-force
enumeration of paths and against autograd, and the host logic of chain.graph_supervisions / GraphSupervision."""
import numpy as np
import pytest
import torch

from pykaldi2_amd import _lib, chain, ops, synth

import num_graph_ref as R
from test_align_graph import PRONS, kaldi_like_lexicon, make_model

PDFS = 60
WORDS = [3, 4]      # both words have two pronunciations; silence is optional around them


def _aligner(tscale=1.0, lscale=0.1, seed=21):
    tree, tm = make_model(7, 2, 1, seed=seed, num_pdfs=PDFS)
    return chain.MappedAligner.from_models(tm, tree, kaldi_like_lexicon(PRONS), disambig=[9, 10], transition_scale=tscale,
                                           self_loop_scale=lscale)


def _min_frames(aligner, words):
    for T in range(1, 60):
        if aligner.compile([words], [T]).status == [chain.ALIGN_OK]:
            return T
    raise AssertionError("no feasible length")


def test_oracle_matches_brute_force():
    aligner = _aligner()
    rng = np.random.default_rng(5)
    Tmin = _min_frames(aligner, WORDS)
    assert aligner.compile([WORDS], [Tmin - 1]).status == [chain.ALIGN_NO_PATH]
    for T in range(Tmin, Tmin + 4):
        g = aligner.compile([WORDS], [T]).export(0)
        x = 2.0 * rng.standard_normal((T, PDFS))
        paths = R.enumerate_paths(g, T)
        assert len(paths) >= (1 if T == Tmin else 4)
        scores = np.asarray([sum(-float(g["weight"][k]) + x[t, g["pdf"][k]] for t, k in enumerate(p)) - float(g["final"][g["dst"][p[-1]]])
                             for p in paths])
        want = scores.max() + np.log(np.exp(scores - scores.max()).sum())
        occ_want = np.zeros((T, g["src"].shape[0]))
        for p, s in zip(paths, scores):
            occ_want[np.arange(T), p] += np.exp(s - want)
        logp, gamma, occ = R.forward_backward(g, x, with_arcs=True)
        assert abs(logp - want) <= 1e-10, (T, logp, want)
        assert np.abs(occ - occ_want).max() <= 1e-10
        assert np.abs(gamma.sum(1) - 1.0).max() <= 1e-10
    # more than one pronunciation and the optional silence take part
    assert len({tuple(g["pdf"][p]) for p in paths}) > 4


def test_oracle_without_stored_occupancies_is_identical():
    """forward_backward keeps occ[T, A] only when asked to (it is hundreds of MB on the large graphs of
    tests/graph_cases.py): the result without it is the one with it, and both are the occupancies summed by pdf."""
    aligner = _aligner()
    rng = np.random.default_rng(7)
    words = [3, 5, 4, 2]
    T = _min_frames(aligner, words) + 9
    g = aligner.compile([words], [T]).export(0)
    x = (2.0 * rng.standard_normal((T, PDFS))).astype(np.float32)
    lp_a, gamma_a, occ = R.forward_backward(g, x, with_arcs=True)
    lp_b, gamma_b = R.forward_backward(g, x)
    assert lp_a == lp_b and np.array_equal(gamma_a, gamma_b)
    want = np.zeros((T, PDFS))
    for t in range(T):
        np.add.at(want[t], g["pdf"], occ[t])
    assert np.array_equal(gamma_b, want) and occ.shape == (T, g["src"].shape[0]) and (occ.sum(1) > 0.999).all()
    # without a path of T frames: log p = -inf and no posterior, on either way through
    T0 = _min_frames(aligner, words) - 1
    lp, gamma, occ = R.forward_backward(g, x[:T0], with_arcs=True)
    assert lp == -np.inf and not gamma.any() and not occ.any()
    lp, gamma = R.forward_backward(g, x[:T0])
    assert lp == -np.inf and not gamma.any()


def test_oracle_gamma_is_autograd_gradient():
    aligner = _aligner(seed=22)
    rng = np.random.default_rng(6)
    T = _min_frames(aligner, WORDS) + 5
    g = aligner.compile([WORDS], [T]).export(0)
    x = torch.from_numpy(2.0 * rng.standard_normal((T, PDFS))).requires_grad_(True)
    lp = R.log_prob_torch(g, x)
    lp.backward()
    logp, gamma = R.forward_backward(g, x.detach().numpy())
    assert abs(logp - float(lp.detach())) <= 1e-9
    assert np.abs(gamma - x.grad.numpy()).max() <= 1e-9


def test_graph_supervisions_status_and_fields():
    aligner = _aligner()
    Tmin = _min_frames(aligner, WORDS)        # (the feasible lengths do not depend on the scales)
    gs = chain.graph_supervisions(aligner, [WORDS, WORDS, [4]], [Tmin + 6, Tmin - 1, 9], weight=0.5)
    assert isinstance(gs, chain.GraphSupervision)
    assert gs.status == [chain.ALIGN_OK, chain.ALIGN_NO_PATH, chain.ALIGN_OK]
    assert gs.frames_per_sequence == [Tmin + 6, Tmin - 1, 9] and gs.num_sequences == 3 and len(gs) == 3
    assert gs.weight == 0.5 and gs.label_dim == aligner.transition_model.num_pdfs()
    assert "no path of %d frames" % (Tmin - 1) in gs.errors[1] and gs.errors[0] == ""
    # both scales default to 0: only the lexicon's costs remain, and the scales are passed through as options
    w0 = gs.graphs.export(0)["weight"]
    lex = kaldi_like_lexicon(PRONS)["weight"]
    sums = {round(float(a + b), 5) for a in np.concatenate([lex, [0.0]]) for b in np.concatenate([lex, [0.0]])}
    assert all(round(float(v), 5) in sums for v in w0)
    w1 = chain.graph_supervisions(aligner, [WORDS], [Tmin + 6], transition_scale=1.0, self_loop_scale=0.1).graphs.export(0)["weight"]
    assert w1.shape == w0.shape and np.abs(w1 - w0).max() > 0.01
    assert np.array_equal(w1, aligner.compile([WORDS], [Tmin + 6]).export(0)["weight"])


def test_out_of_vocabulary_raises():
    aligner = _aligner()
    with pytest.raises(_lib.Pk2Error, match="77"):
        chain.graph_supervisions(aligner, [WORDS, [2, 77]], [40, 40])


def _den_and_opts():
    P = 10
    return chain.DenominatorGraph(synth.den_graph_arcs(20, 100, P, 1), P), chain.ChainTrainingOptions()


def test_mixed_supervision_list_raises_type_error():
    aligner = _aligner()
    gs = chain.graph_supervisions(aligner, [WORDS], [40])
    tree, tm = synth.chain_model(PDFS, seed=1)
    sup = chain.Supervision(dict(num_states=2, frames=1, src=[0], dst=[1], pdf=[0], weight=[0.0], frame_offsets=[0, 1],
                                 final_states=[1], final_weights=[0.0]))
    den, opts = _den_and_opts()
    x = torch.zeros(2, 40, 10)
    with pytest.raises(TypeError, match="mixes"):
        chain.compute_chain_objf_and_deriv(opts, den, [gs, sup], x)
    with pytest.raises(TypeError, match="mixes"):
        ops.ChainObjtiveBatch.apply(x, den, [sup, gs], opts)


def test_graph_entries_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    aligner = _aligner()
    gs = chain.graph_supervisions(aligner, [WORDS], [40])
    den, opts = _den_and_opts()
    x = torch.zeros(1, 40, 10)
    with pytest.raises(_lib.Pk2Error, match="no CPU fallback"):
        chain.compute_chain_objf_and_deriv(opts, den, gs, x)
    with pytest.raises(_lib.Pk2Error, match="no CPU fallback"):
        chain.num_graph_forward_backward(gs, x)
    with pytest.raises(_lib.Pk2Error, match="no CPU fallback"):
        ops.ChainObjtiveFunction.apply(x[0], den, gs, opts)
    with pytest.raises(_lib.Pk2Error, match="no CPU fallback"):
        ops.ChainObjtiveBatch.apply(x, den, gs, opts)


def test_bad_arguments_fail_before_any_launch():
    """Null pointers, too few columns and too small a workspace are refused on the host side of the C entry."""
    aligner = _aligner()
    gs = chain.graph_supervisions(aligner, [WORDS], [40])
    L = _lib.lib()
    h = gs.graphs._h
    need = L.pk2_num_graph_workspace_bytes(h)
    assert need > 0 and L.pk2_num_graph_workspace_bytes(None) == 0
    buf = np.zeros(64, np.float32)          # stands in for every device pointer: nothing is launched
    p = _lib.ptr(buf)
    max_pdf = int(gs.graphs.export(0)["pdf"].max())
    call = lambda packed, P, wsb: L.pk2_num_graph_fwd_bwd(h, packed, p, 0, PDFS, P, 40, 1.0, p, 0, PDFS, p, p, p, wsb, None)   # noqa: E731
    for args, word in (((None, PDFS, need), b"null"), ((p, max_pdf, need), b"columns"), ((p, PDFS, need - 1), b"workspace")):
        rc = call(*args)
        assert rc < 0 and word in L.pk2_last_error(), (rc, L.pk2_last_error())
    den, opts = _den_and_opts()
    rc = L.pk2_chain_objf_and_deriv_graph(den._h, p, 0, PDFS, h, p, 1e-4, 0.0, 0.0, 1.0, p, 0, PDFS, p, p, 1 << 40, None)
    assert rc < 0 and b"pdfs" in L.pk2_last_error()
    rc = L.pk2_chain_objf_and_deriv_graph(den._h, p, 0, PDFS, h, None, 1e-4, 0.0, 0.0, 1.0, p, 0, PDFS, p, p, 1 << 40, None)
    assert rc < 0 and b"null" in L.pk2_last_error()
