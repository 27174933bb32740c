"""Word-boundary alignment, the parts that need no device: word_boundary.int, the strings of the packed
arcs, the frame capacity, the refusals of the C ABI that come before any device work, the sequential restatement
(tests/align_words_ref.py) against utterances whose alignment is known by construction, ctm_lines(times_key=...) and the
start-up refusals of bin/score.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_words_ref as A  # noqa: E402
from pykaldi2_amd import _lib, chain, score  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_boundary_reads_good_files_and_names_the_bad_line(tmp_path):
    good = tmp_path / "word_boundary.int"
    good.write_text("1 nonword\n2 begin\n3 end\n4 internal\n\n7 singleton\n")
    wb = score.WordBoundary.read(str(good))
    assert wb.table.dtype == np.uint8 and wb.table.tolist() == [255, 0, 1, 2, 3, 255, 255, 4]
    assert [wb.category(p) for p in (0, 1, 7, 8, 1000, -1)] == [255, 0, 4, 255, 255, 255]
    assert score.WordBoundary({1: "nonword", 7: "singleton", 2: 1}).table.tolist() == [255, 0, 1, 255, 255, 255, 255, 4]
    for n, text in ((2, "1 nonword\n2 start\n"), (1, "x begin\n"), (3, "1 nonword\n2 begin\n3\n"), (2, "5 end\n5 end\n"),
                    (1, "1 nonword extra\n"), (1, "-1 nonword\n")):
        bad = tmp_path / "bad.int"
        bad.write_text(text)
        with pytest.raises(ValueError, match=r"bad\.int, line %d" % n):
            score.WordBoundary.read(str(bad))
    with pytest.raises(ValueError, match="category"):
        score.WordBoundary({3: "middle"})


def hand_lattice():
    """0 -a-> 1 -b-> 2 (final, string 7 7) and 0 -c-> 3 (final, string 9); state 4 is a dead end and is trimmed."""
    strs = [[1, 2, 3], [4], [5, 6], [8]]
    fstrs = [[], [], [7, 7], [9], []]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    flat = lambda xs: np.asarray([t for x in xs for t in x], np.int32)
    return dict(num_states=5, start=0, src=np.asarray([0, 1, 0, 1], np.int32), dst=np.asarray([1, 2, 3, 4], np.int32),
                word=np.asarray([11, 12, 13, 14], np.int32), graph=np.zeros(4, np.float32), acoustic=np.zeros(4, np.float32),
                final=np.asarray([np.inf, np.inf, 0.0, 0.5, np.inf], np.float32), final_acoustic=np.zeros(5, np.float32),
                tid_off=off(strs), tids=flat(strs), final_tid_off=off(fstrs), final_tids=flat(fstrs))


def test_packed_strings_follow_orig_arc_and_the_finals_carry_their_strings():
    lat = hand_lattice()
    P = score.pack_lattice(lat, "hand")
    off, tids = score.packed_strings(P, lat, "hand")
    assert off.dtype == np.int64 and tids.dtype == np.int32 and off.shape == (P.A + 1,) and off[0] == 0
    by_word = {int(P.word_ids[P.word[a]]): tids[off[a]:off[a + 1]].tolist() for a in range(P.A) if P.word[a]}
    assert by_word == {11: [1, 2, 3], 12: [4], 13: [5, 6]}
    ends = sorted(tids[off[a]:off[a + 1]].tolist() for a in range(P.A) if P.dst[a] == P.S - 1)
    assert ends == [[7, 7], [9]] and all(P.word[a] == 0 for a in range(P.A) if P.dst[a] == P.S - 1)
    strs = sorted(tuple(tids[off[a]:off[a + 1]].tolist()) for a in range(P.A))
    assert strs == [(1, 2, 3), (4,), (5, 6), (7, 7), (9,)]                     # the dead end's arc is gone, both finals are arcs
    assert np.array_equal(np.diff(off), P.arc_len)
    # the archive form gives the same strings
    arcs = [(int(s), int(d), int(w), int(w), (0.0, 0.0, lat["tids"][lat["tid_off"][a]:lat["tid_off"][a + 1]].tolist()))
            for a, (s, d, w) in enumerate(zip(lat["src"], lat["dst"], lat["word"]))]
    finals = [(float(lat["final"][s]), 0.0, lat["final_tids"][lat["final_tid_off"][s]:lat["final_tid_off"][s + 1]].tolist())
              for s in range(5)]
    ark = dict(num_states=5, start=0, arcs=arcs, finals=finals)
    P2 = score.pack_lattice(ark, "hand")
    off2, tids2 = score.packed_strings(P2, ark, "hand")
    assert np.array_equal(off, off2) and np.array_equal(tids, tids2)
    # one transition-id per arc: strings of length 0 or 1
    one = {k: v for k, v in lat.items() if not k.startswith("tid") and not k.startswith("final_tid")}
    one["tid"] = np.asarray([5, 0, 6, 7], np.int32)
    P3 = score.pack_lattice(one, "one")
    off3, tids3 = score.packed_strings(P3, one, "one")
    assert sorted(tuple(tids3[off3[a]:off3[a + 1]].tolist()) for a in range(P3.A)) == [(), (), (), (5,), (6,)]
    bare = {k: v for k, v in one.items() if k != "tid"}
    with pytest.raises(ValueError, match="lattice bare: no transition-id strings"):
        score.packed_strings(score.pack_lattice(bare, "bare"), bare, "bare")


def test_frame_capacity_is_the_longest_path_in_frames():
    lat = hand_lattice()
    P = score.pack_lattice(lat, "hand")
    assert A.frame_capacity(P, P.arc_len) == 6                             # 1 2 3 | 4 | 7 7 against 5 6 | 9
    rng = np.random.default_rng(0)
    model = A.Model("chain")
    utts = [A.make_utterance(rng, model, 3, T=t) for t in (9, 40, 23)]
    paths = [A.cut_path(rng, u) + (float(i), 0.0) for i, u in enumerate(utts)]
    lat = A.make_lattice(paths)
    P = score.pack_lattice(lat)
    assert A.frame_capacity(P, P.arc_len) == 40
    with pytest.raises(ValueError, match="reached at frame"):
        score.state_times(P)                                                   # the state times of such a lattice disagree


def test_the_abi_refuses_without_a_device():
    L = _lib.lib()
    i, off = np.zeros(64, np.int32), np.zeros(8, np.int64)
    ip = _lib.ptr(i)
    assert L.pk2_wordlat_set_strings(None, _lib.ptr(off), ip) == -1 and b"null" in L.pk2_last_error()
    assert L.pk2_wordlat_frame_capacity(None, ip) == -1
    assert L.pk2_wordlat_align_workspace_bytes(None, 0, 1, 1) == 0
    h = C.c_void_p()
    u8 = np.zeros(8, np.uint8)
    assert L.pk2_wordalign_model_create(4, None, ip, _lib.ptr(u8), 4, _lib.ptr(u8), None, C.byref(h)) == -1 and not h
    assert L.pk2_wordalign_model_create(0, ip, ip, _lib.ptr(u8), 4, _lib.ptr(u8), None, C.byref(h)) == -1 and not h
    neg = np.asarray([0, 1, -2, 1, 1], np.int32)
    assert L.pk2_wordalign_model_create(4, ip, _lib.ptr(neg), _lib.ptr(u8), 4, _lib.ptr(u8), None, C.byref(h)) == -1
    assert b"phone -2 of transition-id 2" in L.pk2_last_error() and not h
    cat = np.asarray([0, 1, 9, 255], np.uint8)
    assert L.pk2_wordalign_model_create(4, ip, ip, _lib.ptr(u8), 4, _lib.ptr(cat), None, C.byref(h)) == -1
    assert b"category 9 of phone 2" in L.pk2_last_error() and not h
    assert L.pk2_wordalign_model_destroy(None) == 0
    assert L.pk2_wordlat_align_words(None, None, 0, 1, 1, ip, ip, ip, 64, ip, ip, 1, ip, ip, 1, ip, ip, 1, ip, ip, None) == -1
    assert b"null" in L.pk2_last_error() and not i.any()


def test_align_words_needs_a_topology():
    # the check comes before anything touches a device: a stand-in for the batch is enough
    from pykaldi2_amd.lattice import TransitionModel
    tm = TransitionModel([-1, 0, 0], [0, 1, 1])
    with pytest.raises(ValueError, match="carries no topology"):
        score._AlignModel(tm, score.WordBoundary({1: "nonword"}), "cpu")
    with pytest.raises(ValueError, match="carries no topology"):
        chain.split_to_phones(tm, [1, 2])


@pytest.mark.parametrize("topology", A.TOPOLOGIES)
def test_the_restatement_reproduces_the_truth_by_construction(topology):
    rng = np.random.default_rng(A.TOPOLOGIES.index(topology))
    model = A.Model(topology)
    shapes = [dict(n_words=0), dict(n_words=1, sil_prob=0.0), dict(n_words=1, extra="one"), dict(n_words=4, extra="none"),
              dict(n_words=6, sil_prob=1.0), dict(n_words=9, sil_prob=0.3), dict(n_words=5, T=200), dict(n_words=12, extra="one")]
    if topology == "chain":
        shapes += [dict(n_words=1, sil_prob=0.0, max_pron=1, T=1), dict(n_words=0, T=1), dict(n_words=20, extra="none", max_pron=1)]
    for kw in shapes * 3:
        utt = A.make_utterance(rng, model, **kw)
        ok, phones = chain.split_to_phones(model.trans_model, utt["tids"])
        assert ok and phones == utt["phones"]
        pieces, arc_labels, final = A.cut_path(rng, utt)
        assert [t for p in pieces for t in p] + final == utt["tids"]
        want = A.truth_record(utt, pieces, arc_labels)
        got = A.align_string(model.trans_model, model.word_boundary, utt["tids"], utt["labels"], want["path_times"])
        A.same_record(got, want)
        assert (np.diff(got["times"].reshape(-1)) >= 0).all()               # aligned times cannot overlap


def test_the_restatement_flags_malformed_paths():
    rng = np.random.default_rng(5)
    model = A.Model("bakis_reordered")
    tm, wb = model.trans_model, model.word_boundary
    utt = A.make_utterance(rng, model, 3, sil_prob=1.0, max_pron=3)
    pt = [(i, i + 1) for i in range(4)]
    run = lambda tids, labels, wb_=wb: A.align_string(tm, wb_, tids, labels, pt[:len(labels)])
    assert run(utt["tids"], utt["labels"])["reason"] == 0
    B, I, E, S = (model.variant(0, v) for v in range(4))
    ph = lambda p: model.phone_string(p, [1, 2, 1])
    cut = run(utt["tids"] + ph(S)[:-1], utt["labels"] + [7])                   # ends inside a phone: its last HMM state is missing
    assert cut["status"] == 1 and cut["reason"] & 1 and np.array_equal(cut["times"], cut["path_times"]) and not len(cut["silences"])
    assert run(ph(B) + ph(A.SIL), [7])["reason"] == 2                          # begin without end
    assert run(ph(I) + ph(E), [7])["reason"] == 2                              # internal first
    assert run(ph(S), [7, 8])["reason"] == 4 and run(ph(S) + ph(model.variant(1, 3)), [7])["reason"] == 4
    few = score.WordBoundary({p: c for p, c in zip(model.phones, ["nonword"] + ["begin", "internal", "end", "singleton"] * 5)
                              if p != S})
    r = run(ph(A.SIL) + ph(S), [7], few)                                       # a phone absent from the table
    assert r["reason"] & 8 and r["status"] == 1 and len(r["phones"]) == 2


def test_ctm_lines_prints_the_entry_times_key_names_and_leaves_integer_times_alone():
    sym = {1: "A", 2: "B", 3: "<UNK>"}
    rec = dict(words=[1, 3, 2], conf=np.asarray([0.5, 0.25, 1.0]), times=np.asarray([[0.0, 6.0], [4.0, 8.0], [8.0, 9.0]]),
               aligned=np.asarray([[1, 4], [4, 8], [9, 12]], np.int32))
    assert score.ctm_lines("u", rec, sym, 0.03) == ["u 1 0.000 0.150 A 0.5000", "u 1 0.240 0.030 B 1.0000"]      # as before
    assert score.ctm_lines("u", rec, sym, 0.03, times_key="times") == score.ctm_lines("u", rec, sym, 0.03)
    assert score.ctm_lines("u", rec, sym, 0.03, times_key="aligned") == ["u 1 0.030 0.090 A 0.5000", "u 1 0.270 0.090 B 1.0000"]
    # integer times are printed as they are: no fix_word_times, even where they would overlap
    over = dict(words=[1, 2], conf=[1.0, 1.0], times=np.asarray([[0, 6], [4, 8]], np.int32))
    assert score.ctm_lines("u", over, sym, 1.0) == ["u 1 0.000 6.000 A 1.0000", "u 1 4.000 4.000 B 1.0000"]


@pytest.mark.parametrize("flags,named", [(["-word_boundary", "wb.int", "-model", "final.mdl", "-ctm", "-decode_mbr"], "-decode_mbr"),
                                         (["-word_boundary", "wb.int", "-model", "final.mdl", "-ctm", "-combine", "x.ark"], "-combine"),
                                         (["-word_boundary", "wb.int", "-ctm"], "-model"),
                                         (["-phone_ctm", "-ctm"], "-word_boundary")])
def test_score_cli_refuses_at_start_up(tmp_path, flags, named):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "score.py"), "-lat_file", str(tmp_path / "none.ark"), "-words_txt",
                        str(tmp_path / "none.txt"), "-ref_text", str(tmp_path / "none"), "-out_dir", str(tmp_path / "out")] + flags,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and named in r.stderr and "error" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()
