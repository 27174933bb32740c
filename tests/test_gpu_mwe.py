"""N-best paths and the MWE criterion on the device (lattice_nbest.hip) against the host restatement of tests/mwe_ref.py on
oracle.lattice_ref.decode lattices: costs bit-equal, hypotheses and transition-ids identical and in the same order; loss and
gradient against the reference's formula in float64 on the device's own N-best."""
import numpy as np
import pytest
import torch

import mwe_ref
from oracle import lattice_ref as lr
from pykaldi2_amd import lattice, ops, synth

pytestmark = pytest.mark.gpu

CASES = [
    # words pdfs T seed beam lat_beam ac max_active min_active  (tests/test_gpu_lattice.py::CASES)
    (6, 12, 8, 0, 30.0, 3.0, 1.0, 2 ** 31 - 1, 200),
    (40, 60, 40, 1, 8.0, 4.0, 0.5, 2 ** 31 - 1, 0),
    (200, 150, 60, 2, 13.0, 7.0, 0.1, 300, 200),
    (60, 90, 30, 3, 4.0, 2.0, 1.0, 10000, 40),
    (300, 300, 120, 4, 10.0, 5.0, 0.3, 700, 200),
]


def _setup(case):
    nw, P, T, seed, beam, lb, ac, maxa, mina = case
    rng = np.random.default_rng(seed)
    g = synth.decoding_graph_arcs(nw, P, seed=seed, max_phones=3)
    _, tm = synth.alignment_model(P)
    ll = (2.0 * rng.standard_normal((T, P))).astype(np.float32)
    ref = lr.DecodeGraphRef(g["num_states"], g["start"], g["src"], g["dst"], g["ilabel"], g["weight"], g["final"])
    want = lr.decode(ref, ll, tm.tid2pdf, lr.DecoderOptionsRef(beam, lb, maxa, mina, 0.5, ac))
    A = want.arrays()
    A["start_tok"] = want.start_tok
    o = lattice.LatticeFasterDecoderOptions(beam=beam, lattice_beam=lb, max_active=maxa, min_active=mina)
    rec = lattice.MappedLatticeFasterRecognizer(tm, g, ac, o)
    return g, tm, ll, A, rec


def _same(got, want):
    assert len(got) == len(want)
    for (gl, gt, gc), (wl, wt, wc) in zip(got, want):
        assert np.float32(gc) == np.float32(wc)
        assert gl == wl
        assert np.array_equal(gt, wt)


@pytest.mark.parametrize("grouping", ["lds", "global_memory"])
@pytest.mark.parametrize("labels", ["words", "phones"])
@pytest.mark.parametrize("case", CASES)
def test_nbest_matches_restatement(case, labels, grouping, monkeypatch):
    if grouping == "global_memory":
        monkeypatch.setenv("PK2_NB_CAP", "0")
    g, tm, ll, A, rec = _setup(case)
    lat = rec.decode(torch.from_numpy(ll).cuda())
    assert lat.status[0] == 0
    lab = mwe_ref.link_words(g, A) if labels == "words" else mwe_ref.phone_labels(tm, A)
    lm, am = 1.0, case[6]
    for n in (1, 3, 16, 64):
        for distinct in (False, True):
            got = lat.nbest(n, lm, am, labels, distinct)[0]
            want = mwe_ref.kbest(A, lab, n, lm, am, distinct)
            _same(got, want)


def test_device_words_equal_link_words():
    g, tm, ll, A, rec = _setup(CASES[1])
    lat = rec.decode(torch.from_numpy(ll).cuda())
    E = lat.export(0)
    st = E["tok_state"]
    host = rec.graph.link_words(st[E["link_src"]], st[E["link_dst"]], E["link_tid"], E["link_graph"])
    assert np.array_equal(host, mwe_ref.link_words(g, E))
    # every label the device puts on a hypothesis is the label of one of its links
    for labs, tids, cost in lat.nbest(64, 1.0, 1.0, "words", True)[0]:
        assert set(labs) <= set(host.tolist())


def test_tiny_case_equals_brute_force():
    g, tm, ll, A, rec = _setup(CASES[0])
    lat = rec.decode(torch.from_numpy(ll).cuda())
    words = mwe_ref.link_words(g, A)
    every = mwe_ref.brute_force(A, words, 1.0, 1.0)
    got = lat.nbest(64, 1.0, 1.0, "words", True)[0]
    best = {}
    for labs, tids, cost in every:
        best.setdefault(tuple(labs), cost)
    assert [c for _, _, c in got] == sorted(best.values())[:64]


def _sup(rng, A, lab, n):
    return [int(w) for w in rng.integers(1, max(2, int(lab.max()) + 1), size=n)]


@pytest.mark.parametrize("equal_weight", [False, True])
@pytest.mark.parametrize("phone_level", [False, True])
def test_mwe_matches_formula(equal_weight, phone_level):
    case = CASES[4]
    g, tm, ll, A, rec = _setup(case)
    P, T = case[1], case[2]
    lat = rec.decode(torch.from_numpy(ll).cuda())
    rng = np.random.default_rng(7)
    if phone_level:
        sup, _, _ = synth.phone_tid_alignment(rng, T, tm)
        sup_labels = [p for p, _, _ in __import__("pykaldi2_amd.chain", fromlist=["x"]).split_to_phones(tm, sup)[1]]
    else:
        sup = synth.word_transcript(rng, T, case[0])
        sup_labels = sup
    for distinct in (False, True):
        cfg = dict(lm_weight=1.0, am_weight=case[6], phone_level=phone_level, rand_path=False, num_paths=16,
                   equal_weight=equal_weight, distinct=distinct)
        loss, grad = lat.mwe([sup], cfg)
        hyps = lat.nbest(16, 1.0, case[6], "phones" if phone_level else "words", distinct)[0]
        wl, wg = mwe_ref.mwe_formula(hyps, sup_labels, tm.tid2pdf, T, P, equal_weight)
        assert abs(loss.item() - wl) <= 1e-9 * max(1.0, abs(wl))
        G = grad[0].cpu().numpy().astype(np.float64)
        assert np.abs(G - wg).max() <= 2e-6 * max(1.0, np.abs(wg).max())
        loss2, grad2 = lat.mwe([sup], cfg)
        assert loss2.item() == loss.item() and torch.equal(grad, grad2)     # bit-reproducible


def test_batch_equals_single_calls_and_backward():
    case = CASES[4]
    g, tm, ll, A, rec = _setup(case)
    P = case[1]
    rng = np.random.default_rng(3)
    lens = [120, 77, 101]
    lls = [torch.from_numpy((2.0 * rng.standard_normal((T, P))).astype(np.float32)).cuda() for T in lens]
    sups = [synth.word_transcript(rng, T, case[0]) for T in lens]
    cfg = dict(lm_weight=1.0, am_weight=case[6], phone_level=False, rand_path=False, num_paths=16, equal_weight=False)
    x = torch.zeros(max(lens), len(lens), P, device="cuda")           # time-major, as the BLSTM produces it
    for n, v in enumerate(lls):
        x[:lens[n], n] = v
    pred = x.transpose(0, 1).requires_grad_(True)
    total = ops.MWEBatchFunction.apply(pred, lens, rec, tm, sups, cfg)
    total.backward()
    gb = pred.grad
    s = 0.0
    for n, v in enumerate(lls):
        vv = v.clone().requires_grad_(True)
        loss = ops.MWEFunction.apply(vv, rec, tm, sups[n], cfg)
        loss.backward()
        assert torch.equal(gb[n, :lens[n]], vv.grad)
        assert gb[n, lens[n]:].abs().max().item() == 0.0 if lens[n] < max(lens) else True
        s += loss.item()
    assert np.isfinite(total.item()) and abs(total.item() - s) <= 1e-5 * max(1.0, abs(s))


def test_num_paths_out_of_range_raises():
    g, tm, ll, A, rec = _setup(CASES[0])
    lat = rec.decode(torch.from_numpy(ll).cuda())
    for bad in (0, 65):
        with pytest.raises(ValueError):
            lat.nbest(bad)
