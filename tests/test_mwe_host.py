"""N-best minimum word error (ops.MWEFunction) without a GPU: the host restatement of tests/mwe_ref.py against brute-force
path enumeration on tiny lattices, the phone-label rule against split_to_phones, and the reference's config checks."""
import inspect

import numpy as np
import pytest
import torch

import mwe_ref
from oracle import lattice_ref as lr
from pykaldi2_amd import chain, lattice, ops, synth

# the tiny decodes of tests/test_gpu_lattice.py::CASES (words pdfs T seed beam lat_beam ac max_active min_active)
TINY = [(6, 12, 8, 0, 30.0, 3.0, 1.0, 2 ** 31 - 1, 200), (40, 60, 40, 1, 8.0, 4.0, 0.5, 2 ** 31 - 1, 0),
        (60, 90, 30, 3, 4.0, 2.0, 1.0, 10000, 40)]


def decode_ref(case):
    nw, P, T, seed, beam, lb, ac, maxa, mina = case
    rng = np.random.default_rng(seed)
    g = synth.decoding_graph_arcs(nw, P, seed=seed, max_phones=3)
    tm = synth.transition_model_arrays(P)
    ll = (2.0 * rng.standard_normal((T, P))).astype(np.float32)
    ref = lr.DecodeGraphRef(g["num_states"], g["start"], g["src"], g["dst"], g["ilabel"], g["weight"], g["final"])
    lat = lr.decode(ref, ll, tm["tid2pdf"], lr.DecoderOptionsRef(beam, lb, maxa, mina, 0.5, ac))
    A = lat.arrays()
    A["start_tok"] = lat.start_tok
    return g, A


def _small_enough(A):
    try:
        return mwe_ref.brute_force(A, np.zeros(A["link_src"].shape[0], np.int32))
    except RuntimeError:
        return None


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("case", TINY[:1])
def test_restatement_matches_brute_force(case, distinct):
    g, A = decode_ref(case)
    words = mwe_ref.link_words(g, A)
    assert (words >= 0).all()
    every = mwe_ref.brute_force(A, words, 1.0, 0.5)
    assert every, "no complete path"
    for n in (1, 3, 16, 64):
        got = mwe_ref.kbest(A, words, n, 1.0, 0.5, distinct)
        if distinct:      # best path of each distinct label sequence, the n best of those
            best = {}
            for labs, tids, cost in every:
                best.setdefault(tuple(labs), cost)
            want = sorted(best.values())[:n]
            assert [c for _, _, c in got] == want
            assert len({tuple(h[0]) for h in got}) == len(got)
        else:             # the n best paths, repeated label sequences dropped
            top = every[:n]
            assert len(every) < n or sorted(c for _, _, c in got) == sorted(
                {tuple(h[0]): h[2] for h in reversed(top)}.values())
            seen = []
            for labs, _, _ in top:
                if labs not in seen:
                    seen.append(labs)
            assert [h[0] for h in got] == seen
        for labs, tids, cost in got:       # every path is a real complete path with that cost
            assert tids.shape[0] == A["tok_frame"].max()
            assert any(labs == b[0] and np.array_equal(tids, b[1]) and cost == b[2] for b in every)


def test_phone_label_rule_matches_split_to_phones():
    _, tm = synth.alignment_model(30)
    tab = tm.phone_label_table()
    rng = np.random.default_rng(0)
    for _ in range(5):
        ali, _, _ = synth.phone_tid_alignment(rng, 200, tm)
        ok, pieces = chain.split_to_phones(tm, ali)
        assert ok
        got = [int(tab[t]) for t in ali if tab[t] != 0]
        assert got == [p for p, _, _ in pieces]


def test_phone_labels_need_a_topology():
    tm = lattice.TransitionModel.from_arrays(synth.transition_model_arrays(30))
    with pytest.raises(ValueError):
        tm.phone_label_table()


def test_edit_distance():
    assert mwe_ref.edit_distance([], [1, 2]) == 2
    assert mwe_ref.edit_distance([1, 2, 3], [1, 3]) == 1
    assert mwe_ref.edit_distance([5, 1, 2], [1, 2, 6]) == 2
    assert mwe_ref.edit_distance([1, 2], [2, 1]) == 2


CONFIG = dict(lm_weight=1.0, am_weight=0.1, phone_level=False, rand_path=False, num_paths=16, equal_weight=False)


def test_config_validation():
    assert lattice.mwe_config(CONFIG)["distinct"] is False
    assert lattice.mwe_config(dict(CONFIG, distinct=True))["distinct"] is True
    with pytest.raises(NotImplementedError, match="rand_path"):
        lattice.mwe_config(dict(CONFIG, rand_path=True))
    for key in CONFIG:
        cfg = dict(CONFIG)
        del cfg[key]
        with pytest.raises(KeyError):
            lattice.mwe_config(cfg)
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError):
            lattice.mwe_config(dict(CONFIG, num_paths=bad))


def test_mwe_functions_check_config_before_decoding():
    x = torch.zeros(4, 6)
    with pytest.raises(NotImplementedError, match="rand_path"):
        ops.MWEFunction.apply(x, None, None, [1], dict(CONFIG, rand_path=True))
    with pytest.raises(KeyError):
        ops.MWEBatchFunction.apply(x.unsqueeze(0), [4], None, None, [[1]], {k: v for k, v in CONFIG.items() if k != "am_weight"})
    with pytest.raises(ValueError):
        ops.MWEFunction.apply(x, None, None, [1], dict(CONFIG, num_paths=100))


def test_mwe_functions_have_the_reference_signature():
    assert list(inspect.signature(ops.MWEFunction.forward).parameters) == \
        ["ctx", "loglikes", "asr_decoder", "trans_model", "supervision", "config"]
    assert list(inspect.signature(ops.MWEBatchFunction.forward).parameters) == \
        ["ctx", "prediction", "lengths", "asr_decoder", "trans_model", "supervisions", "config"]
