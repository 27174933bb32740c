"""Word-boundary alignment of best-path word times on the device (csrc/lattice_align_words.hip) against
utterances whose alignment is known by construction and against the sequential restatement (tests/align_words_ref.py).
Every device buffer of the calls is sentinel poisoned and surrounded by checked guard elements (score._DEBUG_GUARD).

The lattices: the true string is cut into arcs at points that are not word boundaries, every label sits on an arc before, on
or after the arc with its phones, some arcs have empty strings, a final weight carries the tail, and worse paths of other
lengths make the state times inconsistent (mbr(times=True) refuses such a lattice)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_words_ref as A  # noqa: E402
import recipe  # noqa: E402
from pykaldi2_amd import _lib, chain, kaldi_io, lattice, score, synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = score.ALIGN_CHUNK
SETTINGS = [(1.0, 0.1, 0.0), (1.0, 0.05, 0.5)]
_MODELS = {}


@pytest.fixture(autouse=True)
def poisoned_buffers():
    score._DEBUG_GUARD = True
    yield
    score._DEBUG_GUARD = False


def model_of(topology):
    if topology not in _MODELS:
        _MODELS[topology] = A.Model(topology)
    return _MODELS[topology]


def lattice_of(rng, model, utt, rivals=1, labels=None):
    """(lattice, pieces, arc labels) with `utt` as the best path and `rivals` worse paths of other lengths."""
    pieces, arc_labels, final = A.cut_path(rng, utt, labels=labels)
    paths = [(pieces, arc_labels, final, 0.0, 0.0)]
    for r in range(rivals):
        other = A.make_utterance(rng, model, int(rng.integers(0, 4)))
        paths.append(A.cut_path(rng, other) + (5000.0 + r, 5.0))
    return A.make_lattice(paths), pieces, arc_labels


def check_against_truth_and_restatement(model, lats, truths, settings=SETTINGS):
    batch = score.WordLatticeBatch(lats)
    recs = batch.align_words(settings, model.trans_model, model.word_boundary, phones=True)
    post = batch.arc_posteriors(settings)
    best = batch.best_path(settings)
    for n, row in enumerate(recs):
        with pytest.raises(ValueError, match="reached at frame"):
            score.state_times(batch.packed[n])
        for g, rec in enumerate(row):
            A.same_record(rec, truths[n])
            A.same_record(rec, A.align_ref(batch, n, post[n][g], model.trans_model, model.word_boundary))
            assert rec["words"] == best[n][g][0] and rec["cost"] == best[n][g][1]
            string = A.best_path_string(batch.packed[n], *batch.strings[n], post[n][g]["backpointer"])[0]
            want = chain.split_to_phones(model.trans_model, string)[1] if string else []
            assert rec["phones"].tolist() == [list(x) for x in want]
            assert int(rec["phones"][:, 2].sum()) == len(string)
    return batch, recs


@pytest.mark.parametrize("topology", A.TOPOLOGIES)
def test_lengths_around_the_wavefront_and_the_chunk(topology):
    model, rng = model_of(topology), np.random.default_rng(10 + A.TOPOLOGIES.index(topology))
    lats, truths = [], []
    for T in (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7):
        if T == 1 and topology != "chain":
            T = 3                                   # the shortest utterance of a three-state topology
        kw = dict(n_words=1, sil_prob=0.0, max_pron=1) if T < 10 else dict(n_words=3)
        utt = A.make_utterance(rng, model, T=T, **kw)
        lat, pieces, arc_labels = lattice_of(rng, model, utt)
        lats.append(lat)
        truths.append(A.truth_record(utt, pieces, arc_labels))
    batch, _ = check_against_truth_and_restatement(model, lats, truths)
    assert batch.frame_cap == [A.frame_capacity(p, p.arc_len) for p in batch.packed]


@pytest.mark.parametrize("topology", A.TOPOLOGIES)
def test_one_word_no_word_cuts_after_every_frame_and_a_long_self_loop_run(topology):
    model, rng = model_of(topology), np.random.default_rng(20 + A.TOPOLOGIES.index(topology))
    utts = [A.make_utterance(rng, model, 1, T=20), A.make_utterance(rng, model, 0, T=30),
            A.make_utterance(rng, model, 300 if topology == "chain" else 14, extra="none"),        # every HMM state one frame
            A.make_utterance(rng, model, 2, T=3 * CHUNK + 7, extra="one")]                          # one run of > 2 chunks
    if topology == "chain":
        # a cut after every frame, and more than a chunk of phones, of arcs and of labels: the carries of every scan
        assert all(d == 1 for _, _, d in utts[2]["phones"]) and len(utts[2]["phones"]) > CHUNK + 64 and len(utts[2]["labels"]) > CHUNK
    assert max(d for _, _, d in utts[3]["phones"]) > 2 * CHUNK
    for seed in range(200):                                                                         # a word across a chunk boundary
        u = A.make_utterance(np.random.default_rng(seed), model, 12, T=2 * CHUNK + 40, sil_prob=0.2)
        if any(b < CHUNK - 2 and e > CHUNK + 2 and len([p for p in u["phones"] if b <= p[1] < e]) > 1 for _, b, e in u["words"]):
            utts.append(u)
            break
    assert len(utts) == 5
    lats, truths = [], []
    for utt in utts:
        lat, pieces, arc_labels = lattice_of(rng, model, utt, rivals=2)
        lats.append(lat)
        truths.append(A.truth_record(utt, pieces, arc_labels))
    assert not len(truths[1]["words"]) and len(truths[1]["silences"]) == 1
    check_against_truth_and_restatement(model, lats, truths)


def test_every_pair_reports_its_own_path_when_the_best_path_flips():
    model, rng = model_of("bakis_reordered"), np.random.default_rng(30)
    ua, ub = A.make_utterance(rng, model, 4, T=90), A.make_utterance(rng, model, 2, T=CHUNK + 30)
    pa, pb = A.cut_path(rng, ua), A.cut_path(rng, ub)
    lat = A.make_lattice([pa + (10.0, 0.0), pb + (0.0, 100.0)])        # am = 1 / 7: 10 < 14.3; am = 1 / 17: 10 > 5.9
    settings = [(1.0, 1.0 / 7, 0.0), (1.0, 1.0 / 17, 0.0), (1.0, 1.0 / 8, 0.0)]
    batch = score.WordLatticeBatch([lat])
    row = batch.align_words(settings, model.trans_model, model.word_boundary, phones=True)[0]
    ta, tb = A.truth_record(ua, pa[0], pa[1]), A.truth_record(ub, pb[0], pb[1])
    assert ta["words"] != tb["words"]
    A.same_record(row[0], ta)
    A.same_record(row[1], tb)
    A.same_record(row[2], ta)
    assert [r["cost"] for r in row] == [10.0, (1.0 / 17) * 100.0, 10.0]


def test_malformed_paths_fall_back_to_the_arcs_times_inside_guarded_buffers():
    model, rng = model_of("bakis_reordered"), np.random.default_rng(40)
    tm, wb = model.trans_model, model.word_boundary
    B, I, E, S = (model.variant(0, v) for v in range(4))
    S2 = model.variant(1, 3)
    ph = lambda p: model.phone_string(p, [1, 2, 1])
    good = A.make_utterance(rng, model, 3, sil_prob=1.0)
    cases = [(good["tids"] + ph(S)[:-1], good["labels"] + [7], 1),           # the string ends inside a phone
             (ph(B) + ph(A.SIL), [7], 2),                                    # begin without end
             (ph(I) + ph(E) + ph(A.SIL), [7], 2),                            # internal first
             (ph(A.SIL) + ph(S), [7, 8], 4),                                 # more labels than word tokens
             (ph(S) + ph(S2) + ph(A.SIL), [7], 4)]                           # fewer
    lats = [lattice_of(rng, model, dict(tids=t, labels=l, words=[]))[0] for t, l, _ in cases]
    batch = score.WordLatticeBatch(lats)
    recs = batch.align_words(SETTINGS, tm, wb, phones=True)                  # _Bufs.check() inside: the guards are untouched
    post = batch.arc_posteriors(SETTINGS)
    for n, (tids, labels, bit) in enumerate(cases):
        for g, rec in enumerate(recs[n]):
            A.same_record(rec, A.align_ref(batch, n, post[n][g], tm, wb))
            assert rec["status"] == 1 and rec["reason"] & bit and rec["words"] == labels
            assert np.array_equal(rec["times"], rec["path_times"]) and len(rec["times"]) == len(labels) and not len(rec["silences"])
            assert rec["phones"][:, 2].sum() == len(tids)
    assert recs[1][0]["reason"] == 2 and recs[3][0]["reason"] == 4 and recs[4][0]["reason"] == 4
    # a phone absent from the table
    few = score.WordBoundary({p: int(wb.table[p]) for p in model.phones if p != S})
    lat = lattice_of(rng, model, dict(tids=ph(A.SIL) + ph(S) + ph(S2), labels=[7, 8], words=[]))[0]
    b2 = score.WordLatticeBatch([lat])
    rec = b2.align_words(SETTINGS[:1], tm, few, phones=True)[0][0]
    A.same_record(rec, A.align_ref(b2, 0, b2.arc_posteriors(SETTINGS[:1])[0][0], tm, few))
    assert rec["status"] == 1 and rec["reason"] & 8 and np.array_equal(rec["times"], rec["path_times"])
    A.same_record(b2.align_words(SETTINGS[:1], tm, wb, phones=True)[0][0],
                  A.align_ref(b2, 0, b2.arc_posteriors(SETTINGS[:1])[0][0], tm, wb))
    assert b2.align_words(SETTINGS[:1], tm, wb)[0][0]["status"] == 0
    # no best path: costs that overflow under the setting's scale
    p = A.cut_path(rng, good)
    b3 = score.WordLatticeBatch([A.make_lattice([p + (3e38, 0.0)], decoy=False)])
    rec = b3.align_words([(1e300, 0.1, 0.0)], tm, wb, phones=True)[0][0]
    assert rec["status"] == 3 and rec["words"] == [] and all(len(rec[k]) == 0 for k in ("times", "path_times", "silences", "phones"))
    assert b3.align_words([(1.0, 0.1, 0.0)], tm, wb)[0][0]["status"] == 0


def test_batches_runs_and_launch_splits_give_the_same_arrays():
    model, rng = model_of("bakis"), np.random.default_rng(50)
    lats = [lattice_of(rng, model, A.make_utterance(rng, model, nw, T=T), rivals=2)[0]
            for nw, T in ((1, 17), (6, 300), (0, 9), (20, 2 * CHUNK + 3), (3, 64))]
    lats[2] = lattice_of(rng, model, dict(tids=model.phone_string(model.variant(0, 0), [2, 1, 1]), labels=[5, 6], words=[]))[0]
    settings = score.sweep()
    assert len(settings) == 33
    batch = score.WordLatticeBatch(lats)
    tm, wb = model.trans_model, model.word_boundary
    first = batch.align_words(settings, tm, wb, phones=True)
    again = batch.align_words(settings, tm, wb, phones=True)
    L = _lib.lib()
    one = lambda n: int(L.pk2_wordlat_workspace_bytes(batch._h, n, 1, 33, -1)) + int(L.pk2_wordlat_align_workspace_bytes(batch._h, n, 1, 33))
    mb = 1.5 * max(one(n) for n in range(5)) / 2 ** 20
    assert len(batch._align_chunks(33, mb)) >= 2 and len(batch._align_chunks(33, 4096)) == 1
    split = batch.align_words(settings, tm, wb, phones=True, workspace_mb=mb)
    alone = [score.WordLatticeBatch([lat]).align_words(settings, tm, wb, phones=True)[0] for lat in lats]
    assert {r["status"] for row in first for r in row} == {0, 1}
    for other in (again, split, alone):
        for ra, rb in zip(first, other):
            for a, b in zip(ra, rb):
                A.same_record(a, b)
                assert a["cost"] == b["cost"]
    with pytest.raises(ValueError, match="more than workspace_mb"):
        batch.align_words(settings, tm, wb, workspace_mb=one(3) / 2 ** 21)


def test_the_abi_refuses_before_the_device_is_touched():
    big, small, rng = model_of("chain"), A.Model("chain", nb=1), np.random.default_rng(60)
    utt = A.make_utterance(rng, big, 5, T=40)
    while max(utt["tids"]) <= small.trans_model.num_transition_ids():
        utt = A.make_utterance(rng, big, 5, T=40)
    lat = lattice_of(rng, big, utt)[0]
    L = _lib.lib()
    buf, i = np.zeros(64, np.float64), np.zeros(4096, np.int32)
    p, ip = _lib.ptr(buf), _lib.ptr(i)
    bare = score.WordLatticeBatch([{k: v for k, v in lat.items() if "tid" not in k}], names=["utt7"])
    with pytest.raises(ValueError, match="lattice utt7: no transition-id strings"):
        bare.align_words(SETTINGS, big.trans_model, big.word_boundary)
    with pytest.raises(ValueError, match="carries no topology"):
        bare.align_words(SETTINGS, lattice.TransitionModel([-1, 0], [0, 1]), big.word_boundary)
    batch = score.WordLatticeBatch([lat])
    P = batch.packed[0]
    m_big = score._AlignModel(big.trans_model, big.word_boundary, batch.device)
    m_small = score._AlignModel(small.trans_model, small.word_boundary, batch.device)

    def align(h=batch._h, m=m_big.h, first=0, count=1, G=1, bp=ip, work=p, work_bytes=None, ws=P.depth, ts=None, ps=None, phones=ip,
              status=ip):
        cap = batch.frame_cap[0] if batch.frame_cap else 64
        need = int(L.pk2_wordlat_align_workspace_bytes(batch._h, 0, 1, 1))
        return L.pk2_wordlat_align_words(h, m, first, count, G, bp, ip, work, need if work_bytes is None else work_bytes, ip, ip, ws,
                                         ip, ip, cap if ts is None else ts, phones, ip, cap if ps is None else ps, status, ip, None)
    assert L.pk2_wordlat_align_workspace_bytes(batch._h, 0, 1, 1) == 0
    assert align(work_bytes=1 << 20) == -1 and b"no strings" in L.pk2_last_error()                    # strings never set
    off, tids = score.packed_strings(P, lat)
    down = off.copy(); down[2] = down[1] - 1
    assert L.pk2_wordlat_set_strings(batch._h, _lib.ptr(down), _lib.ptr(tids)) == -1 and b"decrease" in L.pk2_last_error()
    zero = tids.copy(); zero[3] = 0
    assert L.pk2_wordlat_set_strings(batch._h, _lib.ptr(off), _lib.ptr(zero)) == -1 and b"transition-id 0" in L.pk2_last_error()
    assert align(work_bytes=1 << 20) == -1 and b"no strings" in L.pk2_last_error()                    # a refused upload sets nothing
    batch._upload_strings()
    assert batch.frame_cap == [A.frame_capacity(P, P.arc_len)] and batch.frame_cap[0] >= 40
    assert L.pk2_wordlat_set_strings(batch._h, _lib.ptr(off), _lib.ptr(tids)) == -1 and b"already" in L.pk2_last_error()
    need = int(L.pk2_wordlat_align_workspace_bytes(batch._h, 0, 1, 1))
    assert need == 8 * ((3 * P.depth + 4 * batch.frame_cap[0] + 1) // 2)
    assert L.pk2_wordlat_align_workspace_bytes(batch._h, 0, 2, 1) == 0 and L.pk2_wordlat_align_workspace_bytes(batch._h, 0, 1, 65) == 0
    assert align(m=m_small.h) == -1 and b"the model has" in L.pk2_last_error()                        # a tid beyond the model
    assert align(ws=P.depth - 1) == -1 and b"word_stride" in L.pk2_last_error()
    assert align(ts=batch.frame_cap[0] - 1) == -1 and b"token_stride" in L.pk2_last_error()
    assert align(ps=batch.frame_cap[0] - 1) == -1 and b"phone_stride" in L.pk2_last_error()
    assert align(work_bytes=need - 8) == -1 and b"workspace" in L.pk2_last_error()
    assert align(first=1) == -1 and b"lattices 1..2 of 1" in L.pk2_last_error()
    assert align(G=0) == -1 and align(G=65) == -1 and b"settings" in L.pk2_last_error()
    assert align(bp=None) == -1 and align(work=None) == -1 and align(status=None) == -1 and align(m=None) == -1
    assert b"null" in L.pk2_last_error()
    assert not buf.any() and not i.any()
    # and the batch still aligns
    rec = batch.align_words(SETTINGS[:1], big.trans_model, big.word_boundary)[0][0]
    assert rec["status"] == 0 and [(w, b, e) for w, (b, e) in zip(rec["words"], rec["times"].tolist())] == utt["words"]


def test_decoder_lattices_end_to_end():
    """Two synthetic utterances through the recogniser and the determiniser: the phones of every best path are SplitToPhones
    of its string and fill the utterance; the synthetic lexicon is not position-dependent, so the word level may report
    status 1, and then the times are the arcs' own."""
    Pn = 60
    g = synth.decoding_graph_arcs(40, Pn, seed=4, max_phones=3)
    rec = lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(synth.transition_model_arrays(Pn)), g, 0.2,
                                                lattice.LatticeFasterDecoderOptions(beam=10.0, lattice_beam=4.0))
    rng = np.random.default_rng(3)
    lens = [40, 31]
    ll = np.zeros((2, max(lens), Pn), np.float32)
    for n, Tn in enumerate(lens):
        ll[n, :Tn] = 2.0 * rng.standard_normal((Tn, Pn))
    lat = rec.decode_batch(torch.from_numpy(ll).cuda(), lens)
    dets = [lat.compact_lattice(n, determinize=True) for n in range(2)]
    tm = synth.transition_model_topology(Pn)
    wb = score.WordBoundary({p: "nonword" if p == 1 else "singleton" for p in range(1, Pn // 3 + 1)})
    batch = score.WordLatticeBatch(dets, names=["synth-0", "synth-1"])
    settings = [(1.0, 0.2, 0.0), (1.0, 0.1, 0.5)]
    recs = batch.align_words(settings, tm, wb, phones=True)
    post = batch.arc_posteriors(settings)
    timed = batch.mbr(settings, decode_mbr=False, times=True)
    assert batch.frame_cap == lens
    for n in range(2):
        for g_ in range(2):
            r = recs[n][g_]
            string, labels, pt = A.best_path_string(batch.packed[n], *batch.strings[n], post[n][g_]["backpointer"])
            ok, want = chain.split_to_phones(tm, string)
            print("utt %d setting %d: %d words, %d phones, status %d reason %d" % (n, g_, len(r["words"]), len(want), r["status"], r["reason"]))
            assert len(string) == lens[n] and r["phones"].tolist() == [list(x) for x in want]
            assert int(r["phones"][:, 2].sum()) == lens[n] and r["status"] in (0, 1) and bool(r["reason"] & 1) == (not ok)
            assert np.array_equal(r["path_times"], timed[n][g_]["path_times"]) and r["words"] == labels
            if r["status"] == 1:
                assert np.array_equal(r["times"], r["path_times"])
            A.same_record(r, A.align_ref(batch, n, post[n][g_], tm, wb))


def test_score_cli_writes_aligned_ctm_files(tmp_path):
    model, rng = model_of("bakis_reordered"), np.random.default_rng(70)
    tm, wb = model.trans_model, model.word_boundary
    lats, utts = {}, {}
    for key, nw in (("utt1", 3), ("utt2", 5), ("utt3", 1)):
        utts[key] = A.make_utterance(rng, model, nw, sil_prob=1.0, vocab=5)
        rival = A.make_utterance(rng, model, 2, vocab=5)
        lats[key] = A.make_lattice([A.cut_path(rng, utts[key]) + (0.0, 0.0), A.cut_path(rng, rival) + (60.0, 5.0)], decoy=False)
    lats["utt3"] = A.make_lattice([A.cut_path(rng, dict(tids=model.phone_string(model.variant(0, 0), [1, 1, 1]), labels=[2], words=[]))
                                   + (0.0, 0.0)], decoy=False)                # begin without end: keeps its arc's times
    with kaldi_io.CompactLatticeWriter("ark:" + str(tmp_path / "lat.ark")) as w:
        for k, v in lats.items():
            w[k] = v
    sym = {0: "<eps>", 1: "A", 2: "B", 3: "C", 4: "D", 5: "E"}
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (s, i) for i, s in sym.items()))
    (tmp_path / "text").write_text("".join("%s %s\n" % (k, " ".join(sym[x] for x in utts[k]["labels"])) for k in lats))
    (tmp_path / "word_boundary.int").write_text("".join("%d %s\n" % (p, {v: k for k, v in score.WORD_BOUNDARY_CATEGORIES.items()}[
        int(wb.table[p])]) for p in model.phones))
    recipe.write_transition_model_text(str(tmp_path / "final.mdl"), tm.phone2entry, tm.entries, tm.tuples)

    def run(out, flags):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "score.py"), "-lat_file", str(tmp_path / "lat.ark"),
                            "-words_txt", str(tmp_path / "words.txt"), "-ref_text", str(tmp_path / "text"), "-out_dir",
                            str(tmp_path / out), "-min_lmwt", "9", "-max_lmwt", "10", "-word_ins_penalty", "0.0,1.0", "-ctm",
                            "-frame_shift", "0.03"] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    plain_out = run("plain", [])
    out = run("aligned", ["-word_boundary", str(tmp_path / "word_boundary.int"), "-model", str(tmp_path / "final.mdl"), "-phone_ctm"])
    assert "aligned: 8 of 12 pairs, fallback: 4\n" in out and out.index("aligned:") < out.index("best:")
    assert out.replace("aligned: 8 of 12 pairs, fallback: 4\n", "") == plain_out
    names = ["%d_%s" % st[3] for st in score.sweep(9, 10, (0.0, 1.0))]
    assert sorted(os.listdir(tmp_path / "aligned")) == sorted(os.listdir(tmp_path / "plain") + ["phone_ctm_" + x for x in names])
    batch = score.WordLatticeBatch(list(lats.values()), names=list(lats))
    settings = score.sweep(9, 10, (0.0, 1.0))
    post, conf = batch.arc_posteriors(settings), batch.mbr(settings, decode_mbr=False)
    batch._upload_strings()
    later = 0
    for g, name in enumerate(names):
        for f in os.listdir(tmp_path / "plain"):
            if not f.startswith("ctm_"):
                assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "aligned" / f).read_bytes()
        want, phones = [], []
        for n, key in enumerate(lats):
            ref = A.align_ref(batch, n, post[n][g], tm, wb)
            want += score.ctm_lines(key, dict(ref, conf=conf[n][g]["conf"]), sym, 0.03)
            phones += ["%s 1 %.3f %.3f %d" % (key, b * 0.03, d * 0.03, p) for p, b, d in ref["phones"].tolist()]
        got = (tmp_path / "aligned" / ("ctm_" + name)).read_text().splitlines()
        old = (tmp_path / "plain" / ("ctm_" + name)).read_text().splitlines()
        assert got == want and len(old) == len(got)
        assert (tmp_path / "aligned" / ("phone_ctm_" + name)).read_text().splitlines() == phones
        later += sum(float(a.split()[2]) > float(b.split()[2]) for a, b in zip(got, old))
        assert [a.split()[4:] for a in got] == [b.split()[4:] for b in old]          # the same words and confidences
    assert later > 0                                                                  # words that began inside a silence
