"""Lattice scoring on the device (pykaldi2_amd.score, csrc/lattice_score.hip) against the float64
restatement tests/mbr_ref.py on identical packed lattices.  Every device buffer of the calls is NaN / sentinel poisoned
and surrounded by checked guard elements (score._DEBUG_GUARD).

Tolerances are derived, not measured: alpha(end) and the best-path cost are sums of at most depth terms and log-adds with a
few ulp each (1e-12 relative); p_a = exp of a difference of such sums of magnitude <= ~1e3 (1e-10 absolute); risk,
confidences and bin posteriors are sums of at most A (Q + 1) <= 1e5 products, each with a few 2^-53 relative error, on
values <= Q (1e-9 absolute).  Words, iterations, status and back-pointers must be equal: test_score_host.py holds the
conditions on the inputs that make them well defined, and the fixed cases assert the same conditions here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import kaldi_io, lattice, score, synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = {shape: 0 for shape in R.SHAPES}        # the seeds tests/test_score_host.py has passed
MAX_ERR = {}


@pytest.fixture(autouse=True)
def poisoned_buffers():
    score._DEBUG_GUARD = True
    yield
    score._DEBUG_GUARD = False


def chain(words):
    return R.paths_lattice([(list(words), 1.0)])


def fan_in(n, seed):
    """start -> n middle states -> one join state -> final: a state with n incoming arcs, a level of n states."""
    rng = np.random.default_rng(seed)
    src = [0] * n + list(range(1, n + 1))
    dst = list(range(1, n + 1)) + [n + 1] * n
    A = 2 * n
    final = np.full(n + 2, np.inf, np.float32)
    final[n + 1] = 0.0
    return dict(num_states=n + 2, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
                word=rng.integers(1, 7, A).astype(np.int32), graph=(4.0 * rng.random(A)).astype(np.float32),
                acoustic=(40.0 * rng.random(A)).astype(np.float32), tid=np.ones(A, np.int32), final=final)


def parallel_arcs():
    """Two parallel arcs with the same word between one pair of states, then two different words."""
    return dict(num_states=3, start=0, src=np.asarray([0, 0, 1, 1, 0], np.int32), dst=np.asarray([1, 1, 2, 2, 2], np.int32),
                word=np.asarray([4, 4, 5, 6, 9], np.int32), graph=np.asarray([0.5, 1.25, 0.75, 1.5, 2.0], np.float32),
                acoustic=np.asarray([3.0, 1.0, 2.0, 0.5, 6.0], np.float32), tid=np.ones(5, np.int32),
                final=np.asarray([np.inf, np.inf, 0.25], np.float32))


def all_epsilon():
    return R.paths_lattice([([0, 0, 0], 0.7), ([0, 0], 0.3)])


FIXED = {
    "chain31": lambda: chain(range(1, 32)), "chain32": lambda: chain(range(1, 33)), "all_epsilon": all_epsilon,
    "fan_in70": lambda: fan_in(70, 1), "level40": lambda: R.random_lattice(3, 40, 6, seed=0), "parallel": parallel_arcs,
    # the lane groups of the kernel: Q + 1 = 16 | 18 (groups of 16, then of 32), 22 (32), 32 | 34 (groups of 32, whole waves)
    "groups16_32": lambda: R.random_lattice(18, 3, 6, seed=2), "groups32": lambda: R.random_lattice(18, 3, 6, seed=4),
    "chain15": lambda: chain(range(1, 16)), "chain16": lambda: chain(range(1, 17)),
}
_REF = {}


def ref(P, st, **kw):
    key = (id(P), tuple(st[:3]), tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = (P, R.mbr(P, st, **kw))
    return _REF[key][1]


def conditions_hold(o):
    m = o["margins"]
    return m["sum"] <= 1e-12 and m["tie"] >= 1e-12 and m["argmax"] >= 1e-6 and m["best_path"] >= 1e-9


def note(name, value):
    MAX_ERR[name] = max(MAX_ERR.get(name, 0.0), float(value))


def check_pair(P, st, post, rec, want, bins=0):
    z = want["post"]
    assert post["status"] == 0
    assert abs(post["alpha_end"] - z["alpha_end"]) <= 1e-12 * max(1.0, abs(z["alpha_end"]))
    assert np.abs(post["post"] - z["post"]).max() <= 1e-10
    assert post["words"] == z["words"] and np.array_equal(post["backpointer"], z["backpointer"])
    assert abs(post["cost"] - z["cost"]) <= 1e-12 * max(1.0, abs(z["cost"]))
    note("p_a", np.abs(post["post"] - z["post"]).max())
    assert rec["words"] == want["words"] and rec["iterations"] == want["iterations"] and rec["status"] == want["status"]
    assert abs(rec["risk"] - want["risk"]) <= 1e-9
    note("risk", abs(rec["risk"] - want["risk"]))
    if len(want["words"]):
        assert np.abs(rec["conf"] - want["conf"]).max() <= 1e-9
        note("conf", np.abs(rec["conf"] - want["conf"]).max())
    if bins:
        assert len(rec["bins"]) == len(want["bins"])
        for got, exp in zip(rec["bins"], want["bins"]):
            assert [w for w, _ in got] == [w for w, _ in exp]
            assert max(abs(a[1] - b[1]) for a, b in zip(got, exp)) <= 1e-9
            note("bins", max(abs(a[1] - b[1]) for a, b in zip(got, exp)))


def run_case(lat, bins=2):
    P = score.pack_lattice(lat)
    batch = score.WordLatticeBatch([P])
    posts = batch.arc_posteriors(R.SETTINGS)[0]
    recs = batch.mbr(R.SETTINGS, bins=bins)[0]
    bests = batch.best_path(R.SETTINGS)[0]
    for g, st in enumerate(R.SETTINGS):
        want = ref(P, st, bins=bins)
        assert conditions_hold(want), want["margins"]
        check_pair(P, st, posts[g], recs[g], want, bins)
        assert bests[g] == (posts[g]["words"], posts[g]["cost"])
    return P, recs


@pytest.mark.parametrize("shape", R.SHAPES)
def test_generator_lattices_against_the_restatement(shape):
    run_case(R.random_lattice(*shape, seed=SEEDS[shape]))
    print("largest errors so far:", MAX_ERR)


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_cases_against_the_restatement(name):
    P, recs = run_case(FIXED[name]())
    if name == "chain31":
        assert 2 * len(recs[0]["words"]) + 2 == 64 and recs[0]["words"] == list(range(1, 32))
    if name == "chain32":
        assert 2 * len(recs[0]["words"]) + 2 == 66 and abs(recs[0]["risk"]) <= 1e-9 and np.abs(recs[0]["conf"] - 1).max() <= 1e-9
    if name == "all_epsilon":
        assert recs[0]["words"] == [] and recs[0]["iterations"] == 1 and recs[0]["bins"] == []
    if name == "groups16_32":
        assert [2 * len(r["words"]) + 2 for r in recs] == [16, 18, 18]
    if name == "groups32":
        assert [2 * len(r["words"]) + 2 for r in recs] == [22, 18, 18]
    if name == "fan_in70":
        assert int(np.diff(P.in_off).max()) == 70
    if name == "level40":
        assert int(np.diff(P.level_off).max()) == 40
    print("largest errors so far:", MAX_ERR)


def test_hand_made_lattices_max_iter_and_best_path_confidences():
    a, b, c, x, y = 1, 2, 3, 7, 8
    P1 = score.pack_lattice(R.paths_lattice([([a, b], 0.6), ([a, c], 0.4)]))
    P2 = score.pack_lattice(R.paths_lattice([([x, y], 0.4), ([a, b], 0.35), ([a, c], 0.25)]))
    st = [(1.0, 1.0, 0.0)]
    batch = score.WordLatticeBatch([P1, P2])
    r1, r2 = (row[0] for row in batch.mbr(st))
    assert r1["words"] == [a, b] and abs(r1["risk"] - 0.4) <= 1e-6 and np.abs(r1["conf"] - [1.0, 0.6]).max() <= 1e-6
    assert r2["words"] == [a, y] and abs(r2["risk"] - 1.0) <= 1e-6 and r2["iterations"] == 2 and r2["status"] == 0
    assert [w for w, _ in batch.best_path(st)[1]] == [[x, y]]
    # max_iter = 1 where two E-steps are needed: not converged, the 1-best with its own statistics
    one = batch.mbr(st, max_iter=1)[1][0]
    want = R.mbr(P2, st[0], max_iter=1)
    assert one["status"] == 1 and one["iterations"] == 1 and one["words"] == [x, y] == want["words"]
    assert abs(one["risk"] - want["risk"]) <= 1e-9 and np.abs(one["conf"] - want["conf"]).max() <= 1e-9
    # decode_mbr = False: the best path's confidences, no update
    conf = batch.mbr(st, decode_mbr=False, bins=3)[1][0]
    want = R.mbr(P2, st[0], decode_mbr=False, bins=3)
    assert conf["status"] == 0 and conf["iterations"] == 1 and conf["words"] == [x, y]
    assert np.abs(conf["conf"] - want["conf"]).max() <= 1e-9 and np.abs(conf["conf"] - 0.4).max() <= 1e-6
    assert [[w for w, _ in bn] for bn in conf["bins"]] == [[w for w, _ in bn] for bn in want["bins"]]
    # the Python layer's refusals
    for kw in (dict(max_iter=0), dict(bins=9), dict(bins=-1), dict(max_iter=1.5)):
        with pytest.raises(ValueError):
            batch.mbr(st, **kw)
    with pytest.raises(ValueError):
        batch.mbr([(1.0, float("inf"), 0.0)])
    with pytest.raises(ValueError):
        batch.best_path(st * 65)
    with pytest.raises(ValueError, match="workspace_mb"):
        batch.mbr(st, workspace_mb=0.0001)


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra["words"] == rb["words"] and ra["iterations"] == rb["iterations"] and ra["status"] == rb["status"]
        assert ra["risk"] == rb["risk"] and np.array_equal(ra["conf"], rb["conf"]) and ra.get("bins") == rb.get("bins")


def test_batches_runs_and_launch_splits_give_the_same_bits():
    lats = [score.pack_lattice(R.random_lattice(*shape, seed=SEEDS[shape])) for shape in ((8, 4, 5), (2, 1, 2), (20, 8, 8), (3, 2, 3))]
    batch = score.WordLatticeBatch(lats)
    whole = batch.mbr(R.SETTINGS, bins=2)
    again = batch.mbr(R.SETTINGS, bins=2)
    posts = batch.arc_posteriors(R.SETTINGS)
    for n, P in enumerate(lats):
        single = score.WordLatticeBatch([P])
        _same(whole[n], single.mbr(R.SETTINGS, bins=2)[0])
        _same(whole[n], again[n])
        for a, b in zip(posts[n], single.arc_posteriors(R.SETTINGS)[0]):
            assert np.array_equal(a["post"], b["post"]) and a["alpha_end"] == b["alpha_end"] and a["cost"] == b["cost"]
    # a budget that cuts six lattices into three launches
    six = [score.pack_lattice(R.random_lattice(8, 4, 5, seed=s)) for s in range(6)]
    b6 = score.WordLatticeBatch(six)
    G = len(R.SETTINGS)
    one = max(score._lib.lib().pk2_wordlat_workspace_bytes(b6._h, n, 1, G, 0) for n in range(6))
    mb = 2.3 * one / (1 << 20)
    assert len(b6._chunks(G, 0, mb)) == 3 and len(b6._chunks(G, 0, 4096)) == 1
    for ra, rb in zip(b6.mbr(R.SETTINGS), b6.mbr(R.SETTINGS, workspace_mb=mb)):
        _same(ra, rb)


def test_35_lattices_times_33_settings_in_one_call():
    lats = [score.pack_lattice(R.random_lattice(3, 2, 3, seed=s)) for s in range(35)]
    settings = score.sweep()
    batch = score.WordLatticeBatch(lats)
    res = batch.mbr(settings)
    best = batch.best_path(settings)
    assert len(res) == 35 and all(len(row) == 33 for row in res) and len(batch._chunks(33, 0, 4096)) == 1
    for P, row, brow in zip(lats, res, best):
        for st, rec, (bw, bc) in zip(settings, row, brow):
            want = R.mbr(P, st)
            assert abs(bc - want["post"]["cost"]) <= 1e-12 * max(1.0, abs(bc))
            if conditions_hold(want):
                assert rec["words"] == want["words"] and rec["status"] == want["status"] and bw == want["post"]["words"]
                assert abs(rec["risk"] - want["risk"]) <= 1e-9


def test_edit_distance_at_the_lane_chunk_edges():
    rng = np.random.default_rng(1)
    lens = (0, 1, 63, 64, 65, 200)
    hyps, refs = [], []
    for a in lens:
        for b in lens:
            hyps.append(rng.integers(1, 5, a).tolist())
            refs.append(rng.integers(1, 5, b).tolist())
    got = score.edit_distance(hyps, refs)
    assert got.dtype == np.int32 and got.tolist() == [R.edit_distance(h, r) for h, r in zip(hyps, refs)]
    assert score.wer(hyps, refs) == (int(got.sum()), sum(len(r) for r in refs))


def test_decoder_lattices_end_to_end():
    """Two synthetic utterances through the recogniser and the determiniser, then scored: against the restatement on the
    same dicts.  Agreement of the 1-best with the decoder's is printed, not asserted (near-ties are the decoder's business)."""
    Pn = 60
    g = synth.decoding_graph_arcs(40, Pn, seed=4, max_phones=3)
    tm = synth.transition_model_arrays(Pn)
    rec = lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(tm), g, 0.2,
                                                lattice.LatticeFasterDecoderOptions(beam=10.0, lattice_beam=4.0))
    rng = np.random.default_rng(3)
    lens = [40, 31]
    ll = np.zeros((2, max(lens), Pn), np.float32)
    for n, T in enumerate(lens):
        ll[n, :T] = 2.0 * rng.standard_normal((T, Pn))
    lat = rec.decode_batch(torch.from_numpy(ll).cuda(), lens)
    dets = [lat.compact_lattice(n, determinize=True) for n in range(2)]
    packed = [score.pack_lattice(d, "synth-%d" % n) for n, d in enumerate(dets)]
    batch = score.WordLatticeBatch(packed)
    settings = [(1.0, 0.2, 0.0), (1.0, 0.1, 0.5)]
    posts, recs = batch.arc_posteriors(settings), batch.mbr(settings, bins=2)
    for n, P in enumerate(packed):
        for g_, st in enumerate(settings):
            want = R.mbr(P, st, bins=2)
            print("utt %d setting %s: %d states %d arcs, margins %s, 1-best == decoder's: %s" %
                  (n, st, P.S, P.A, want["margins"], posts[n][g_]["words"] == list(dets[n]["best_words"])))
            assert abs(posts[n][g_]["alpha_end"] - want["post"]["alpha_end"]) <= 1e-12 * max(1.0, abs(want["post"]["alpha_end"]))
            assert np.abs(posts[n][g_]["post"] - want["post"]["post"]).max() <= 1e-10
            assert abs(recs[n][g_]["risk"] - want["risk"]) <= 1e-9 or not conditions_hold(want)
            if conditions_hold(want):
                check_pair(P, st, posts[n][g_], recs[n][g_], want, 2)


def test_score_cli_on_a_written_archive(tmp_path):
    a, b, c, x, y = 1, 2, 3, 7, 8
    lats = {"utt1": R.paths_lattice([([a, b], 0.6), ([a, c], 0.4)]),
            "utt2": R.paths_lattice([([x, y], 0.4), ([a, b], 0.35), ([a, c], 0.25)]),
            "utt4": R.paths_lattice([([a], 1.0)])}
    with kaldi_io.CompactLatticeWriter("ark:" + str(tmp_path / "lat.ark")) as w:
        for k, v in lats.items():
            w[k] = v
    sym = {0: "<eps>", a: "A", b: "B", c: "C", x: "<UNK>", y: "Y"}
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (s, i) for i, s in sym.items()))
    (tmp_path / "text").write_text("utt1 A <NOISE> C\nutt2 A Y Y\nutt3 B B\n")
    for mbr_flag in ([], ["-decode_mbr"]):
        out_dir = tmp_path / ("out" + str(len(mbr_flag)))
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "score.py"), "-lat_file", str(tmp_path / "lat.ark"),
                              "-words_txt", str(tmp_path / "words.txt"), "-ref_text", str(tmp_path / "text"), "-out_dir",
                              str(out_dir), "-min_lmwt", "9", "-max_lmwt", "10", "-word_ins_penalty", "0.0,1.0"] + mbr_flag,
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        names = sorted(os.listdir(out_dir))
        assert names == sorted(["hyp_%d.%s.txt" % (l, p) for l in (9, 10) for p in ("0.0", "1.0")] +
                               ["result_%d_%s" % (l, p) for l in (9, 10) for p in ("0.0", "1.0")])
        refs = {"utt1": ["A", "C"], "utt2": ["A", "Y", "Y"]}
        totals = []
        for st in score.sweep(9, 10, (0.0, 1.0)):
            lmwt, wip = st[3]
            total = 2                                           # utt3 has no lattice: its two words are errors
            lines = (out_dir / ("result_%d_%s" % (lmwt, wip))).read_text().splitlines()
            assert len(lines) == (4 if mbr_flag else 3) * 2
            for key in ("utt1", "utt2"):
                P = score.pack_lattice(lats[key])
                want = R.mbr(P, st) if mbr_flag else dict(words=R.posteriors(P, st)["words"])
                hyp = [sym[w_] for w_ in want["words"] if sym[w_] != "<UNK>"]
                err = R.edit_distance(hyp, refs[key]) if hyp else len(refs[key])
                total += err
                assert "reco: %s %s" % (key, " ".join(hyp)) in [l.rstrip() for l in lines]
                assert "%s err: %d ref_len: %d" % (key, err, len(refs[key])) in lines
                assert (" ".join([key] + hyp)) in (out_dir / ("hyp_%d.%s.txt" % (lmwt, wip))).read_text().splitlines()
            totals.append((total, lmwt, wip))
        best = min(totals, key=lambda t: t[0])                   # min keeps the first of equal totals
        last = run.stdout.strip().splitlines()[-1]
        assert last == "best: LMWT=%d wip=%s errors=%d ref_words=7 WER=%.2f%%" % (best[1], best[2], best[0], 100.0 * best[0] / 7)
        assert "no reference for utt4" in run.stdout and "no lattice for utt3" in run.stdout
