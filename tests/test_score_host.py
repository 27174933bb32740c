"""Lattice scoring, host side: the packer of pykaldi2_amd.score on its three input forms, the float64
restatement tests/mbr_ref.py on the hand-made lattices, the conditions under which the GPU test may compare discrete
outputs (tests/test_gpu_score.py uses exactly the lattices that pass here), the refusals of the C ABI and of the Python
layer that need no device, and the word error count against a plain DP."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import _lib, kaldi_io, score  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def check_packed(P):
    """Topological order, level order and both CSR forms of a packed lattice."""
    assert P.S >= 2 and P.A >= 1 and P.src.shape == P.dst.shape == P.word.shape == P.graph.shape == P.acoustic.shape == (P.A,)
    level = np.zeros(P.S, np.int64)
    for a in range(P.A):                                   # arcs are sorted by destination, so sources are final here
        assert P.src[a] < P.dst[a]
        level[P.dst[a]] = max(level[P.dst[a]], level[P.src[a]] + 1)
    assert (np.diff(level) >= 0).all() and level[0] == 0 and level[-1] == P.depth and (level[1:] > 0).all()
    assert (level[:-1] < P.depth).all()
    assert P.level_off.shape == (P.depth + 2,)
    for lev in range(P.depth + 1):
        assert (level[P.level_off[lev]:P.level_off[lev + 1]] == lev).all() and P.level_off[lev + 1] > P.level_off[lev]
    assert P.level_off[-1] == P.S
    assert (np.diff(P.dst) >= 0).all() and (np.diff(P.orig_arc)[np.diff(P.dst) == 0] > 0).all()
    for s in range(P.S):
        assert (P.dst[P.in_off[s]:P.in_off[s + 1]] == s).all()
        out = P.out_idx[P.out_off[s]:P.out_off[s + 1]]
        assert (P.src[out] == s).all() and (np.diff(out) > 0).all()
    assert P.in_off[-1] == P.A and P.out_off[-1] == P.A and sorted(P.out_idx.tolist()) == list(range(P.A))
    assert P.in_off[1] == 0 and (np.diff(P.in_off)[1:] > 0).all() and (np.diff(P.out_off)[:-1] > 0).all()
    assert P.word_ids[0] == 0 and (np.diff(P.word_ids) > 0).all() and P.W == P.word_ids.size
    for w in range(P.W):
        arcs = P.word_arcs[P.word_off[w]:P.word_off[w + 1]]
        assert (P.word[arcs] == w).all() and (np.diff(arcs) > 0).all()
    assert P.word_off[-1] == P.A and P.cap == min(1023, 2 * P.depth + 1)


def _as_det(lat):
    d = dict(lat)
    d["final_acoustic"] = np.where(np.isfinite(lat["final"]), np.float32(0.25), np.float32(np.inf)).astype(np.float32)
    return d


def test_packer_on_the_three_input_forms(tmp_path):
    lat = R.random_lattice(8, 4, 5, seed=0)           # several finals, a dead-end branch, an unreachable state
    P = score.pack_lattice(lat, "raw")
    check_packed(P)
    finals = int(np.isfinite(lat["final"]).sum())
    assert finals == 4 and P.S == 1 + 8 * 4 + 1                         # dead end and unreachable state are gone, one end
    assert P.A == lat["src"].size - 2 + finals                          # their two arcs too; one epsilon arc per final
    assert (P.word[P.dst == P.S - 1] == 0).all() and (P.acoustic[P.dst == P.S - 1] == 0).all()
    assert sorted(P.graph[P.dst == P.S - 1].tolist()) == sorted(lat["final"][np.isfinite(lat["final"])].tolist())
    assert P.word_ids.tolist() == sorted(set([0] + lat["word"][:-2].tolist()))
    assert (P.word_ids[P.word][:P.A - finals] == lat["word"][P.orig_arc[:P.A - finals]]).all()
    # determinised form: the finals carry an acoustic cost
    D = score.pack_lattice(_as_det(lat), "det")
    check_packed(D)
    assert (D.acoustic[D.dst == D.S - 1] == np.float32(0.25)).all() and np.array_equal(D.src, P.src)
    # archive form, through the writer and the reader
    with kaldi_io.CompactLatticeWriter("ark:" + str(tmp_path / "l.ark")) as w:
        w["u0"] = lat
    (key, ark), = list(kaldi_io.read_compact_lattice_ark(str(tmp_path / "l.ark")))
    K = score.pack_lattice(ark, key)
    check_packed(K)
    assert (K.S, K.A, K.depth, K.W) == (P.S, P.A, P.depth, P.W) and np.array_equal(K.word_ids, P.word_ids)
    for st in R.SETTINGS:
        a, b = R.posteriors(P, st), R.posteriors(K, st)
        assert a["words"] == b["words"] and a["cost"] == b["cost"] and abs(a["alpha_end"] - b["alpha_end"]) < 1e-12


def test_packer_word_map_keeps_the_order_of_the_ids():
    lat = R.paths_lattice([([900, 5], 0.5), ([5, 70000], 0.3), ([12], 0.2)])
    P = score.pack_lattice(lat)
    check_packed(P)
    assert P.word_ids.tolist() == [0, 5, 12, 900, 70000] and P.depth == 3 and P.cap == 7


def test_packer_refuses_cycles_and_empty_lattices():
    lat = R.paths_lattice([([1, 2, 3], 1.0)])
    cyc = dict(lat, src=np.append(lat["src"], 2).astype(np.int32), dst=np.append(lat["dst"], 1).astype(np.int32),
               word=np.append(lat["word"], 4).astype(np.int32), graph=np.append(lat["graph"], 0).astype(np.float32),
               acoustic=np.append(lat["acoustic"], 0).astype(np.float32), tid=np.append(lat["tid"], 1).astype(np.int32))
    with pytest.raises(ValueError, match="lattice utt7: cycle"):
        score.pack_lattice(cyc, "utt7")
    nofinal = dict(lat, final=np.full(lat["num_states"], np.inf, np.float32))
    with pytest.raises(ValueError, match="lattice utt8: no path"):
        score.pack_lattice(nofinal, "utt8")
    empty = dict(num_states=0, start=0, src=np.zeros(0, np.int32), dst=np.zeros(0, np.int32), word=np.zeros(0, np.int32),
                 graph=np.zeros(0, np.float32), acoustic=np.zeros(0, np.float32), final=np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="lattice utt9: empty"):
        score.pack_lattice(empty, "utt9")
    with pytest.raises(ValueError, match="lattice x: not a"):
        score.pack_lattice(dict(num_states=1), "x")


def test_restatement_on_the_hand_made_lattices():
    a, b, c, x, y = 1, 2, 3, 7, 8
    o = R.mbr(score.pack_lattice(R.paths_lattice([([a, b], 0.6), ([a, c], 0.4)])), (1.0, 1.0, 0.0))
    assert o["post"]["words"] == [a, b] and o["words"] == [a, b] and o["status"] == 0
    assert abs(o["risk"] - 0.4) < 1e-6 and np.abs(o["conf"] - [1.0, 0.6]).max() < 1e-6      # float32 rounding of -log p
    o = R.mbr(score.pack_lattice(R.paths_lattice([([x, y], 0.4), ([a, b], 0.35), ([a, c], 0.25)])), (1.0, 1.0, 0.0))
    assert o["post"]["words"] == [x, y] and o["words"] == [a, y]                              # not a path of the lattice
    assert abs(o["risk"] - 1.0) < 1e-6 and o["iterations"] == 2 and o["status"] == 0
    one = R.mbr(score.pack_lattice(R.paths_lattice([([x, y], 0.4), ([a, b], 0.35), ([a, c], 0.25)])), (1.0, 1.0, 0.0), max_iter=1)
    assert one["words"] == [x, y] and one["status"] == 1 and one["iterations"] == 1


# Seed 0 of every shape passes the conditions below (no seed had to be skipped); tests/test_gpu_score.py uses the same.
SEEDS = {shape: 0 for shape in R.SHAPES}


@pytest.mark.parametrize("shape", R.SHAPES)
def test_generator_lattices_meet_the_conditions_for_comparing_discrete_outputs(shape):
    """Conditions on the inputs, not tolerances: with them the device and the restatement must take the same decisions."""
    P = score.pack_lattice(R.random_lattice(*shape, seed=SEEDS[shape]))
    check_packed(P)
    for st in R.SETTINGS:
        o = R.mbr(P, st, bins=2)
        m = o["margins"]
        assert m["sum"] <= 1e-12, m            # |sum_w gamma(q)[w] - 1| <= 1e-12 (Q + 1)
        assert m["tie"] >= 1e-12, m            # every compared difference of the decision rule is away from tau
        assert m["argmax"] >= 1e-6, m
        assert m["best_path"] >= 1e-9, m
        assert o["status"] == 0 and len(o["conf"]) == len(o["words"])


def test_sweep_and_settings_refusals():
    s = score.sweep()
    assert len(s) == 33 and s[0] == (1.0, 1.0 / 7, 0.0, (7, 0.0)) and s[1][3] == (7, 0.5) and s[-1][3] == (17, 1.0)
    assert [x[3] for x in score.sweep(9, 10, (0.0, 1.0))] == [(9, 0.0), (9, 1.0), (10, 0.0), (10, 1.0)]
    with pytest.raises(ValueError):
        score.sweep(0, 3)
    with pytest.raises(ValueError):
        score.sweep(5, 4)
    with pytest.raises(ValueError, match="1..64 settings"):
        score._settings_array([(1.0, 0.1, 0.0)] * 65)
    with pytest.raises(ValueError, match="1..64 settings"):
        score._settings_array([])
    with pytest.raises(ValueError, match="finite"):
        score._settings_array([(1.0, float("nan"), 0.0)])
    with pytest.raises(ValueError):
        score.edit_distance([[1]], [[1], [2]], device="cpu")
    with pytest.raises(ValueError, match="1023"):
        score.edit_distance([[1]], [[1] * 1024], device="cpu")


def test_abi_refuses_bad_arguments_before_the_device_is_touched():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pk2hip.h")).read()
    for name, val in (("SETTINGS", score.MAX_SETTINGS), ("POSITIONS", score.MAX_POSITIONS), ("BINS", score.MAX_BINS)):
        assert "#define PK2_WORDLAT_MAX_%s %d\n" % (name, val) in hdr
    st = np.asarray([[1.0, 0.1, 0.0]] * 65)
    buf = np.zeros(64, np.float64)                 # stands for every device pointer: the refusals come before any use
    p, i = _lib.ptr(buf), np.zeros(64, np.int32)
    ip = _lib.ptr(i)

    def best(h=p, settings=st, G=1):
        return L.pk2_wordlat_best_path(h, 0, 1, _lib.ptr(settings) if settings is not None else None, G, p, 512, ip, 4, ip, p, p,
                                       None, None, ip, None)

    def mbr(h=p, settings=st, G=1, max_iter=10, bins=0, words=ip):
        return L.pk2_wordlat_mbr(h, 0, 1, _lib.ptr(settings) if settings is not None else None, G, 1, max_iter, bins, p, 512,
                                 words, p, 4, ip, p, ip, ip, ip, ip, p, 16, None)
    assert best(h=None) == INVALID and b"null" in L.pk2_last_error()
    assert best(settings=None) == INVALID
    assert best(G=0) == INVALID and best(G=65) == INVALID and b"settings" in L.pk2_last_error()
    bad = st.copy(); bad[0, 1] = np.inf
    assert best(settings=bad) == INVALID and b"non-finite" in L.pk2_last_error()
    assert mbr(h=None) == INVALID and mbr(words=None) == INVALID and mbr(settings=None) == INVALID
    assert mbr(G=0) == INVALID and mbr(G=65) == INVALID
    assert mbr(bins=-1) == INVALID and mbr(bins=9) == INVALID and b"bins" in L.pk2_last_error()
    assert mbr(max_iter=0) == INVALID and b"max_iter" in L.pk2_last_error()
    bad[0, 1], bad[0, 2] = 0.1, np.nan
    assert mbr(settings=bad) == INVALID and b"non-finite" in L.pk2_last_error()
    assert L.pk2_wordlat_workspace_bytes(None, 0, 1, 1, 0) == 0
    assert L.pk2_edit_distance_batch(None, p, p, p, 1, ip, None) == INVALID and L.pk2_edit_distance_batch(p, p, p, p, -1, ip, None) == INVALID
    assert L.pk2_wordlat_destroy(None) == 0
    # a malformed packed lattice is refused by the host-side validation: an arc that does not go up a level
    P = score.pack_lattice(R.paths_lattice([([1, 2], 0.6), ([1, 3], 0.4)]))
    off = lambda n: np.asarray([0, n], np.int64)
    src = P.src.copy(); src[-1] = P.S - 1
    h = C.c_void_p()

    def create(src_):
        return L.pk2_wordlat_create(1, _lib.ptr(off(P.S)), _lib.ptr(off(P.A)), _lib.ptr(off(P.depth + 2)), _lib.ptr(off(P.W + 1)),
                                    _lib.ptr(src_), _lib.ptr(P.dst), _lib.ptr(P.word), _lib.ptr(P.graph), _lib.ptr(P.acoustic),
                                    _lib.ptr(P.in_off), _lib.ptr(P.out_off), _lib.ptr(P.out_idx), _lib.ptr(P.level_off),
                                    _lib.ptr(P.word_ids), _lib.ptr(P.word_off), _lib.ptr(P.word_arcs), None, C.byref(h))
    assert create(src) == INVALID and b"malformed" in L.pk2_last_error() and not h.value
    assert create(None) == INVALID and not h.value


def test_wer_against_a_plain_dp():
    rng = np.random.default_rng(0)
    hyps = [rng.integers(1, 6, n).tolist() for n in (0, 1, 5, 9, 30, 0, 64, 65)]
    refs = [rng.integers(1, 6, n).tolist() for n in (4, 1, 7, 9, 25, 0, 63, 70)]
    want = [R.edit_distance(h, r) for h, r in zip(hyps, refs)]
    assert score.edit_distance(hyps, refs, device="cpu").tolist() == want
    assert want[0] == 4 and want[5] == 0                   # an empty hypothesis counts len(ref), as utt_wer.py does
    assert score.wer(hyps, refs, device="cpu") == (sum(want), sum(len(r) for r in refs))
