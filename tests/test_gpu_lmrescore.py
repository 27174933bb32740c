"""N-gram LM rescoring on the device (pykaldi2_amd.score.rescore_lm, csrc/lattice_lmrescore.hip) against the
pure-Python restatement tests/lmrescore_ref.py.  Every integer and every float32 bit of the composed lattice is a function of
the inputs, so the comparison is exact.  Every device buffer of the calls is sentinel poisoned and surrounded by checked
guard elements (score._DEBUG_GUARD)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmrescore_ref as R  # noqa: E402
import mbr_ref  # noqa: E402
from pykaldi2_amd import _lib, ngram, score  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def poisoned_buffers():
    score._DEBUG_GUARD = True
    yield
    score._DEBUG_GUARD = False


_LMS = {}


def lms(vocab, order, seed, density=0.5):
    """(device LM, restatement's LM) of one seeded set of n-grams, made once."""
    key = (vocab, order, seed, density)
    if key not in _LMS:
        ngrams, bos, eos = R.random_lm(vocab, order, seed, density)
        _LMS[key] = (ngram.NgramLM.from_ngrams(ngrams, bos, eos, order), R.RefLM(ngrams, bos, eos, order))
    return _LMS[key]


def check(lats, lm, ref, scale, unk_id=None, **kw):
    got = score.rescore_lm(lats, [(lm, scale)], **kw)
    assert len(got) == len(lats)
    for i, (g, lat) in enumerate(zip(got, lats)):
        want = R.compose(score.pack_lattice(lat), ref, scale, unk_id)
        assert R.same_composition(g, want) is None, (i, R.same_composition(g, want))
    return got


def raw(src, dst, word, finals, seed=0):
    rng = np.random.default_rng(seed)
    n, A = max(max(src), max(dst)) + 1, len(src)
    final = np.full(n, np.inf, np.float32)
    final[list(finals)] = (2.0 * rng.random(len(finals))).astype(np.float32)
    return dict(num_states=n, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                word=np.asarray(word, np.int32), graph=(4.0 * rng.random(A)).astype(np.float32),
                acoustic=(40.0 * rng.random(A)).astype(np.float32), tid=np.ones(A, np.int32), final=final)


def fan_in(n, seed, dup=False):
    """start -> n states by n distinct words (a seeded permutation) -> one join by epsilon arcs (two parallel ones per
    state with dup) -> final.  With a bigram LM in which every word is a context the join gets n pairs from n (2 n)
    candidates whose h' are not in candidate order."""
    words = [int(w) for w in 1 + np.random.default_rng(seed).permutation(n)]
    mids = list(range(1, n + 1))
    src, dst, word = [0] * n + mids * (2 if dup else 1), mids + [n + 1] * (n * (2 if dup else 1)), words + [0] * (n * (2 if dup else 1))
    return raw(src, dst, word, [n + 1], seed)


def context_lms(n):
    """Bigram LM over the words 1..n in which every word is a context: (w, </s>) for every w."""
    if ("ctx", n) not in _LMS:
        rng = np.random.default_rng(n)
        bos, eos = n + 1, n + 2
        ngrams = {(w,): (float(-0.5 - rng.random()), float(-0.1 - rng.random()) if w <= n else None) for w in range(1, n + 3)}
        for w in range(1, n + 1):
            ngrams[(w, eos)] = (float(-0.2 - rng.random()), None)
        _LMS[("ctx", n)] = (ngram.NgramLM.from_ngrams(ngrams, bos, eos, 2), R.RefLM(ngrams, bos, eos, 2))
    return _LMS[("ctx", n)]


@pytest.mark.parametrize("order", [2, 3])
def test_random_lattices(order):
    lats = [mbr_ref.random_lattice(d, w, v, seed=0) for d, w, v in mbr_ref.SHAPES]
    for vocab in sorted(set(v for _, _, v in mbr_ref.SHAPES)):
        lm, ref = lms(vocab, order, 20 + order)
        check([l for l, s in zip(lats, mbr_ref.SHAPES) if s[2] == vocab], lm, ref, 1.0)


def test_four_gram_that_backs_off_three_times():
    """(1 2 3) is a state; the word 2 after it has no 4-gram, no trigram after (2 3) and no bigram after (3): three backoff
    weights, then the unigram.  (1 2) has a single child; the unigram range is searched at its first (1) and its last
    (</s> = 5) place."""
    bos, eos = 4, 5
    ngrams = {(1,): (-0.7, -0.31), (2,): (-0.9, -0.22), (3,): (-1.1, -0.43), (bos,): (-99.0, -0.15), (eos,): (-1.3, None),
              (1, 2): (-0.4, -0.27), (2, 3): (-0.5, -0.33), (3, 1): (-0.6, None), (bos, 3): (-0.8, None),
              (1, 2, 3): (-0.3, -0.52), (2, 3, 1): (-0.35, None), (1, 2, 3, 1): (-0.2, None)}
    lm, ref = ngram.NgramLM.from_ngrams(ngrams, bos, eos, 4), R.RefLM(ngrams, bos, eos, 4)
    h = ref.node_of[(1, 2, 3)]
    assert ref.arc(ref.arc(ref.arc(ref.start, 1)[1], 2)[1], 3)[1] == h and ref.backoffs_taken(h, 2) == 3
    assert ref.child_begin[ref.node_of[(1, 2)] + 1] - ref.child_begin[ref.node_of[(1, 2)]] == 1
    assert ref.word[ref.child_begin[0]] == 1 and ref.word[ref.child_begin[1] - 1] == eos
    lat = mbr_ref.paths_lattice([([1, 2, 3, 2], 0.5), ([3, 1], 0.3), ([2, 3, 1], 0.2)])
    got, = check([lat], lm, ref, 1.5)
    # the cost of that arc: three backoff weights and the unigram, added in this order in float64
    want = ((float(ref.backoff[h]) + float(ref.backoff[ref.node_of[(2, 3)]])) + float(ref.backoff[ref.node_of[(3,)]])) + \
        float(ref.cost[ref.node_of[(2,)]])
    assert ref.arc(h, 2)[0] == want
    a = int(np.flatnonzero((got["state_h"][got["src"]] == h) & (got["word"] == 2))[0])
    P = score.pack_lattice(lat)
    assert got["graph"][a] == np.float32(np.float64(P.graph[got["orig_arc"][a]]) + 1.5 * want)


def test_fixed_lattices():
    lm, ref = lms(6, 3, 31)
    all_eps = mbr_ref.paths_lattice([([0, 0, 0], 0.7), ([0, 0], 0.3)])
    parallel = raw([0, 0, 1, 1, 0], [1, 1, 2, 2, 2], [4, 4, 5, 6, 2], [2])
    got = check([all_eps, parallel], lm, ref, 1.0)
    assert got[0]["num_states"] == score.pack_lattice(all_eps).S          # epsilons keep the LM state
    lm32, ref32 = lms(32, 2, 32, density=0.1)
    check([mbr_ref.paths_lattice([(list(range(1, 33)), 1.0)])], lm32, ref32, -1.0)


@pytest.mark.parametrize("n", [63, 64, 65, 1025, score.LMRESCORE_SORT_LDS - 1, score.LMRESCORE_SORT_LDS, score.LMRESCORE_SORT_LDS + 1])
def test_fan_in(n):
    """The join's candidates: one wave (<= 64), the workgroup's sort in LDS (<= LMRESCORE_SORT_LDS), in the workspace above."""
    lm, ref = context_lms(score.LMRESCORE_SORT_LDS + 1)
    got, = check([fan_in(n, n)], lm, ref, 1.0)
    assert got["num_states"] == 2 * n + 2 and got["src"].size == 3 * n


@pytest.mark.parametrize("n", [100, 2100])
def test_fan_in_with_equal_keys(n):
    """Two parallel epsilon arcs per state: 2 n candidates in n runs of two equal h' -- the sorts must be stable."""
    lm, ref = context_lms(score.LMRESCORE_SORT_LDS + 1)
    got, = check([fan_in(n, n, dup=True)], lm, ref, 1.0)
    assert got["num_states"] == 2 * n + 2 and got["src"].size == 4 * n


def test_two_thousand_final_states():
    n = 2000
    lm, ref = lms(6, 2, 41)
    words = [int(w) for w in np.random.default_rng(3).integers(1, 7, n)]
    got, = check([raw([0] * n, list(range(1, n + 1)), words, list(range(1, n + 1)), 5)], lm, ref, 1.0)
    assert int((got["dst"] == got["num_states"] - 1).sum()) == n


def test_unknown_words():
    ngrams, bos, eos = R.random_lm(4, 2, 51)
    ref = R.RefLM(ngrams, bos, eos, 2)
    lat = mbr_ref.paths_lattice([([1, 9, 2], 0.6), ([3, 8], 0.4)])          # 8 and 9 are not in the LM
    with pytest.raises(ValueError, match=r"uttA.*word id 8|word id 8.*uttA"):
        score.rescore_lm([lat], [(ngram.NgramLM.from_ngrams(ngrams, bos, eos, 2), 1.0)], names=["uttA"])
    got, = check([lat], ngram.NgramLM.from_ngrams(ngrams, bos, eos, 2, unk_id=4), ref, 1.0, unk_id=4)
    assert sorted(set(got["word"])) == [0, 1, 2, 3, 8, 9]                   # the lattice keeps its own words


def _ragged():
    return [mbr_ref.random_lattice(8, 4, 5, 3), fan_in(70, 1), mbr_ref.paths_lattice([([1, 2], 1.0)]),
            mbr_ref.random_lattice(20, 8, 5, 1), fan_in(5, 2)]


def test_ragged_batch_equals_single_calls_and_a_second_run():
    lm, ref = context_lms(score.LMRESCORE_SORT_LDS + 1)
    lats = _ragged()
    together = check(lats, lm, ref, 0.5)
    again = score.rescore_lm(lats, [(lm, 0.5)])
    for i, lat in enumerate(lats):
        single, = score.rescore_lm([lat], [(lm, 0.5)])
        assert R.same_composition(single, together[i]) is None and R.same_composition(again[i], together[i]) is None


def test_exact_room_and_one_less():
    """The middle lattice of three gets exactly the states it needs (status 0), then one state less (status 2: counts 0,
    guards intact -- checked inside the launch helper --, neighbours right); rescore_lm retries it with twice the room."""
    n = 40
    lm, ref = context_lms(score.LMRESCORE_SORT_LDS + 1)
    lats = [mbr_ref.paths_lattice([([1, 2, 3], 1.0)]), fan_in(n, 7), mbr_ref.paths_lattice([([4], 0.5), ([5, 6], 0.5)])]
    batch = score.WordLatticeBatch(lats, names=["left", "middle", "right"])
    want = [R.compose(p, ref, 1.0) for p in batch.packed]
    S, A = batch.packed[1].S, batch.packed[1].A
    need = want[1]["num_states"]
    assert (S, A, need, want[1]["src"].size) == (n + 3, 2 * n + 1, 2 * n + 2, 3 * n)
    word_dev = _lib.h2d(score._lm_words(batch, lm), batch.device)
    for room, status in ((need, 0), (need - 1, 2)):
        expand = (room + 0.5) / S
        assert int(expand * S) == room and int(expand * A) >= 3 * n           # the states bind, the arcs fit
        assert all(int(expand * p.S) >= w["num_states"] for p, w in zip(batch.packed[::2], want[::2]))
        res = score._lmrescore_launch(batch, 0, 3, lm, word_dev, 1.0, expand)
        assert [r[0] for r in res] == [0, status, 0]
        for i in (0, 1, 2):
            if res[i][0] == 0:
                got = score._composed_dict(batch.packed[i], lats[i], res[i][1], res[i][2])
                assert R.same_composition(got, want[i]) is None
            else:
                assert res[i][1] is None
    small = (need - 0.5) / S
    got = score.rescore_lm(lats, [(lm, 1.0)], expand=small, max_expand=2 * small)
    assert all(R.same_composition(g, w) is None for g, w in zip(got, want))
    with pytest.raises(ValueError, match=r"middle \(%d states, %d arcs\)" % (S, A)):
        score.rescore_lm(lats, [(lm, 1.0)], expand=small, max_expand=1.5 * small, names=["left", "middle", "right"])
    # the arcs bind: a lattice of 300 final states needs 2 x 300 arcs and 302 states
    fin = raw([0] * 300, list(range(1, 301)), [1 + i % 6 for i in range(300)], list(range(1, 301)))
    b2 = score.WordLatticeBatch([fin])
    w2 = R.compose(b2.packed[0], ref, 1.0)
    wd2 = _lib.h2d(score._lm_words(b2, lm), b2.device)
    for room, status in ((600, 0), (599, 2)):
        expand = (room + 0.5) / b2.packed[0].A
        assert int(expand * b2.packed[0].A) == room and (status == 2 or int(expand * b2.packed[0].S) >= w2["num_states"])
        (st, states, arcs), = score._lmrescore_launch(b2, 0, 1, lm, wd2, 1.0, expand)
        assert st == status
        if st == 0:
            assert R.same_composition(score._composed_dict(b2.packed[0], fin, states, arcs), w2) is None


def test_best_path_of_the_rescored_batch_and_a_changed_one_best():
    lm, ref = lms(5, 3, 103)
    lats = [mbr_ref.random_lattice(8, 4, 5, 3), mbr_ref.random_lattice(8, 4, 5, 5)]
    settings = score.sweep(9, 11, (0.0, 0.5))
    batch = score.WordLatticeBatch(lats)
    new = batch.rescore_lm(lm, 1.0)
    before, after = batch.best_path(settings), new.best_path(settings)
    for i, lat in enumerate(lats):
        P = score.pack_lattice(lat)
        C = R.compose(P, ref, 1.0)
        assert R.same_composition(new.source[i], C) is None
        PC = score.pack_lattice(C)
        for g, st in enumerate(settings):
            want = mbr_ref.posteriors(PC, st)
            assert after[i][g][0] == want["words"]
            assert abs(after[i][g][1] - want["cost"]) <= 1e-12 * abs(want["cost"])
    # the new LM changes the 1-best of the first lattice -- in the restatement, so that the device's change means something
    st = (1.0, 0.1, 0.0)
    P = score.pack_lattice(lats[0])
    w0 = mbr_ref.posteriors(P, st)
    w1 = mbr_ref.posteriors(score.pack_lattice(R.compose(P, ref, 1.0)), st)
    assert w0["words"] != w1["words"] and min(w0["margin"], w1["margin"]) > 1e-3
    assert batch.best_path([st])[0][0][0] == w0["words"] and new.best_path([st])[0][0][0] == w1["words"]
    assert before[0] != after[0]


def test_two_lms_in_sequence_return_the_costs():
    """[(lm, -1), (lm, +1)]: the recipe's shape.  The lattice keeps its size and every graph cost comes back to 2 float32 ulp
    at the largest magnitude it went through (tests/test_lmrescore_host.py derives the bound)."""
    lm, ref = lms(5, 3, 103)
    lat = mbr_ref.random_lattice(8, 4, 5, 1)
    one, = score.rescore_lm([lat], [(lm, -1.0)])
    two, = score.rescore_lm([lat], [(lm, -1.0), (lm, 1.0)])
    assert two["num_states"] == one["num_states"] and two["src"].size == one["src"].size
    g, c, fg = lat["graph"], lat["acoustic"], lat["final"]
    orig = np.concatenate([g, fg[np.isfinite(fg)]])[two["input_arc"]]
    cmax = (ref.order - 1) * float(ref.backoff.max()) + float(ref.cost.max())      # no LM cost is larger: the intermediate's size
    bound = 2.0 * np.spacing((np.abs(orig) + cmax).astype(np.float32)).astype(np.float64)
    assert (np.abs(two["graph"].astype(np.float64) - orig.astype(np.float64)) <= bound).all()
    assert np.array_equal(two["acoustic"], np.concatenate([c, np.zeros(int(np.isfinite(fg).sum()), np.float32)])[two["input_arc"]])


def test_abi_refuses_bad_arguments_before_the_device():
    lm, _ = lms(5, 2, 22)
    batch = score.WordLatticeBatch([mbr_ref.paths_lattice([([1, 2], 1.0)])])
    L = _lib.lib()
    word_dev = _lib.h2d(score._lm_words(batch, lm), batch.device)
    bufs = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(6)]
    work = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def call(h_lm=None, scale=1.0, expand=2.0, work_bytes=8 * 4096, rooms=(10, 10), words=word_dev, count=1):
        return L.pk2_wordlat_lmrescore(batch._h, 0, count, lm.handle("cuda") if h_lm is None else h_lm, _lib.ptr(words), scale, expand,
                                       _lib.ptr(work), work_bytes, _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), rooms[0],
                                       _lib.ptr(bufs[3]), rooms[1], _lib.ptr(bufs[4]), _lib.stream_ptr())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(bufs[4][0]) == 0
    for kw in (dict(scale=float("nan")), dict(scale=float("inf")), dict(expand=0.0), dict(expand=float("nan")), dict(work_bytes=16),
               dict(rooms=(2, 10)), dict(rooms=(10, 2)), dict(words=None), dict(count=2), dict(h_lm=0)):
        assert call(**kw) < 0, kw
    assert L.pk2_wordlat_lmrescore_workspace_bytes(batch._h, 0, 2, 2.0) == 0
    assert L.pk2_wordlat_lmrescore_workspace_bytes(batch._h, 0, 1, 1e12) == 0
