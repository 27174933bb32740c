"""Word times and CTM output of lattice scoring, host side: state times of pykaldi2_amd.score on the three
lattice forms, the float64 restatement tests/ctm_ref.py against values computed by hand, the one-best clean-up, the CTM
lines, and the refusals of the new C ABI entries that need no device.  (The refusals that need a batch made by
pk2_wordlat_create -- a negative arc length, short strides -- are in tests/test_gpu_ctm.py: the batch cannot be made
without a device.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctm_ref as T  # noqa: E402
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import _lib, kaldi_io, score  # noqa: E402

INVALID = -1
ONE = (1.0, 1.0, 0.0)


def with_lengths(lat, arc_len, final_len):
    """`lat` (raw form) with transition-id strings of the given lengths; final_len per state (0 where not final)."""
    out = {k: v for k, v in lat.items() if k != "tid"}
    n = int(lat["num_states"])
    out["tid_off"] = np.concatenate([[0], np.cumsum(arc_len)]).astype(np.int64)
    out["tids"] = np.ones(int(np.sum(arc_len)), np.int32)
    out["final_acoustic"] = np.zeros(n, np.float32)
    out["final_tid_off"] = np.concatenate([[0], np.cumsum(final_len)]).astype(np.int64)
    out["final_tids"] = np.ones(int(np.sum(final_len)), np.int32)
    return out


def test_state_times_on_the_three_forms_and_on_inconsistent_lengths(tmp_path):
    raw = R.random_lattice(8, 4, 5, seed=0)
    lat = T.timed(raw, 0)
    P = score.pack_lattice(lat, "timed")
    t = score.state_times(P, lat, "timed")
    assert t.dtype == np.int32 and t.shape == (P.S,) and t[0] == 0 and t[-1] == 10 * P.depth
    assert np.array_equal(t, T.state_times(P, lat)) and np.array_equal(t, score.state_times(P))
    assert np.array_equal(P.arc_len, T.arc_lengths(P, lat))
    lev = np.searchsorted(P.level_off, np.arange(P.S), side="right") - 1
    assert ((t >= 10 * lev) & (t < 10 * lev + 6))[:-1].all()
    # the archive form, through the writer and the reader: the strings are Python tuples there
    with kaldi_io.CompactLatticeWriter("ark:" + str(tmp_path / "l.ark")) as w:
        w["u0"] = lat
    (key, ark), = list(kaldi_io.read_compact_lattice_ark(str(tmp_path / "l.ark")))
    K = score.pack_lattice(ark, key)
    tk = score.state_times(K, ark, key)
    assert np.array_equal(tk, T.state_times(K, ark)) and sorted(tk.tolist()) == sorted(t.tolist()) and tk[-1] == t[-1]
    # the one-tid form: every arc one frame, the finals none -- consistent on a chain, and equal to the same lengths as strings
    ch = R.paths_lattice([([1, 2, 3], 1.0)])
    C1 = score.pack_lattice(ch)
    assert score.state_times(C1, ch).tolist() == [0, 1, 2, 3, 3]
    chs = with_lengths(ch, [1, 1, 1], [0, 0, 0, 0])
    assert score.state_times(score.pack_lattice(chs), chs).tolist() == [0, 1, 2, 3, 3]
    # random_lattice as it is: one tid per arc and arcs that skip levels -- packing works, times are refused
    Pr = score.pack_lattice(raw, "utt5")
    skip = (lev[Pr.dst] - lev[Pr.src] > 1) & (Pr.dst != Pr.S - 1)
    assert Pr.S == P.S and skip.any()
    with pytest.raises(ValueError, match=r"lattice utt5: state \d+ is reached at frame \d+ and at frame \d+"):
        score.state_times(Pr, raw, "utt5")
    with pytest.raises(ValueError):
        T.state_times(Pr, raw)
    first = int(Pr.dst[np.flatnonzero(skip)].min())        # states in order: the first one with a skipping arc is named
    try:
        score.state_times(Pr, raw, "utt5")
    except ValueError as e:
        assert "state %d " % first in str(e)
    # a form without strings
    bare = {k: v for k, v in raw.items() if k != "tid"}
    Pb = score.pack_lattice(bare, "utt6")
    assert Pb.arc_len is None and np.array_equal(Pb.src, Pr.src)
    with pytest.raises(ValueError, match="lattice utt6: no transition-id strings"):
        score.state_times(Pb, bare, "utt6")
    with pytest.raises(ValueError, match="no transition-id strings"):
        score.state_times(Pb)


def test_restatement_on_a_chain_gives_the_arcs_own_times():
    lat = with_lengths(R.paths_lattice([([1, 2, 3], 1.0)]), [3, 5, 2], [0, 0, 0, 4])
    P = score.pack_lattice(lat)
    t = score.state_times(P, lat)
    assert t.tolist() == [0, 3, 8, 10, 14]
    o = T.mbr_times(P, ONE, t, bins=1)
    assert o["words"] == [1, 2, 3] and o["times"].tolist() == [[0.0, 3.0], [3.0, 8.0], [8.0, 10.0]]
    assert o["path_times"].dtype == np.int32 and o["path_times"].tolist() == [[0, 3], [3, 8], [8, 10]]
    assert o["bin_times"] == [[(0.0, 3.0)], [(3.0, 8.0)], [(8.0, 10.0)]]


def test_restatement_two_paths_with_the_same_words_give_posterior_weighted_means():
    lat = with_lengths(R.paths_lattice([([1, 2], 0.6), ([1, 2], 0.4)]), [4, 6, 7, 3], [0, 0, 0, 0, 0])
    P = score.pack_lattice(lat)
    t = score.state_times(P, lat)
    assert t[-1] == 10
    c1, c2 = (float(np.float32(-np.log(p))) for p in (0.6, 0.4))       # the graph costs are float32
    p1 = 1.0 / (1.0 + np.exp(c1 - c2))
    p2 = 1.0 - p1
    o = T.mbr_times(P, ONE, t)
    assert o["words"] == [1, 2] and np.abs(o["conf"] - 1.0).max() <= 1e-12
    want = np.asarray([[0.0, 4 * p1 + 7 * p2], [4 * p1 + 7 * p2, 10.0]])
    assert np.abs(o["times"] - want).max() <= 1e-12 and abs(want[0, 1] - 5.2) < 1e-6
    assert o["path_times"].tolist() == [[0, 4], [4, 10]]               # the best path's own boundary


def test_restatement_a_repeated_word_gets_a_time_pair_per_position():
    lat = with_lengths(R.paths_lattice([([5, 5, 5], 1.0)]), [2, 3, 4], [0, 0, 0, 1])
    P = score.pack_lattice(lat)
    o = T.mbr_times(P, ONE, score.state_times(P, lat))
    assert o["words"] == [5, 5, 5] and o["times"].tolist() == [[0.0, 2.0], [2.0, 5.0], [5.0, 9.0]]


@pytest.mark.parametrize("shape", R.SHAPES)
def test_restatement_statistics_reproduce_gamma_and_stay_inside_the_utterance(shape):
    lat = T.timed(R.random_lattice(*shape, seed=0), 0)
    P = score.pack_lattice(lat)
    t = score.state_times(P, lat)
    for st in R.SETTINGS:
        o = T.mbr_times(P, st, t, bins=2)
        s = o["stats"]
        assert np.abs(s["G1"][1:] - s["gamma"][1:]).max(initial=0.0) <= 1e-12
        every = np.concatenate([o["times"].ravel()] + [np.ravel(b) for b in o["bin_times"]])
        every = every[every != -1.0]
        assert every.min(initial=0.0) >= 0.0 and every.max(initial=0.0) <= float(t[-1])
        assert (o["times"][:, 0] <= o["times"][:, 1]).all() and (o["time_gamma"] >= 0.1).all()
        assert len(o["bin_times"]) == len(o["bins"]) and [len(b) for b in o["bin_times"]] == [len(b) for b in o["bins"]]
        for bn, bt in zip(o["bins"], o["bin_times"]):
            for (w, v), x in zip(bn, bt):
                assert x == (-1.0, -1.0) if (w == 0 or v <= 0) else 0.0 <= x[0] <= x[1]


def test_fix_word_times_on_hand_made_rows():
    f = score.fix_word_times
    src = np.asarray([[0.0, 5.0], [4.0, 8.0]])
    assert f(src).tolist() == [[0.0, 4.5], [4.5, 8.0]] and src.tolist() == [[0.0, 5.0], [4.0, 8.0]]     # a copy
    # a chain of overlaps, left to right: (0,6),(4,5) meet at 5; then (5,5),(3,9) meet at 4 and the middle word's begin follows
    assert f([[0, 6], [4, 5], [3, 9]]).tolist() == [[0.0, 5.0], [4.0, 4.0], [4.0, 9.0]]
    assert f([[3, 2]]).tolist() == [[3.0, 3.0]]                                    # b > e
    assert f([[0, 5], [-1, -1], [4, 8]]).tolist() == [[0.0, 4.5], [-1.0, -1.0], [4.5, 8.0]]
    assert f([[-1, -1], [2, 1]]).tolist() == [[-1.0, -1.0], [2.0, 2.0]]
    assert f(np.zeros((0, 2))).shape == (0, 2) and f([[1, 2], [2, 3]]).tolist() == [[1.0, 2.0], [2.0, 3.0]]


def test_ctm_lines_format_and_dropping():
    sym = {1: "A", 7: "<UNK>", 2: "B", 3: "C"}
    rec = dict(words=[1, 7, 2, 3, 99], conf=np.asarray([0.9, 0.5, 0.25, 0.7, 1.0]),
               times=np.asarray([[0.0, 50.0], [50.0, 60.0], [56.0, 100.0], [-1.0, -1.0], [100.0, 120.0]]))
    assert score.ctm_lines("utt1", rec, sym) == ["utt1 1 0.000 0.500 A 0.9000", "utt1 1 0.580 0.420 B 0.2500",
                                                 "utt1 1 1.000 0.200 99 1.0000"]
    assert score.ctm_lines("u", rec, sym, frame_shift=0.03, channel="A", drop=()) == [
        "u A 0.000 1.500 A 0.9000", "u A 1.500 0.240 <UNK> 0.5000", "u A 1.740 1.260 B 0.2500", "u A 3.000 0.600 99 1.0000"]
    assert score.ctm_lines("u", dict(words=[], conf=np.zeros(0), times=np.zeros((0, 2))), sym) == []


def test_new_abi_entries_refuse_bad_arguments_before_the_device_is_touched():
    L = _lib.lib()
    st = np.asarray([[1.0, 0.1, 0.0]])
    buf = np.zeros(64, np.float64)                 # stands for every device pointer and for a batch nothing was uploaded to
    p, i = _lib.ptr(buf), np.zeros(64, np.int32)
    ip = _lib.ptr(i)

    def mbr_times(h=p, times=p, path=ip, bins=0, bin_times=None):
        return L.pk2_wordlat_mbr_times(h, 0, 1, _lib.ptr(st), 1, 1, 10, bins, p, 512, ip, p, 4, ip, p, ip, ip, ip, ip, p, 16,
                                       times, bin_times, path, 4, None)
    assert L.pk2_wordlat_set_times(None, ip) == INVALID and b"null" in L.pk2_last_error()
    assert L.pk2_wordlat_set_times(p, None) == INVALID and b"null" in L.pk2_last_error()
    assert L.pk2_wordlat_set_times(p, ip) == INVALID and b"not a batch" in L.pk2_last_error()
    assert L.pk2_wordlat_times_workspace_bytes(None, 0, 1, 1, 0) == 0
    assert mbr_times(h=None) == INVALID and b"null" in L.pk2_last_error()
    assert mbr_times(times=None) == INVALID and mbr_times(path=None) == INVALID and b"null" in L.pk2_last_error()
    assert mbr_times() == INVALID and b"no state times" in L.pk2_last_error()          # times never set
    assert not buf.any() and not i.any()
