"""The restatement of the lattice oracle (tests/oracle_ref.py) against an enumeration of every path of the
lattice, and score.lattice_depth on a lattice with known strings.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
import oracle_ref as O  # noqa: E402
from pykaldi2_amd import score  # noqa: E402

SEEDS = range(6)
PLAIN_LIMIT = 2000      # distinct word sequences up to which mbr_ref.edit_distance itself runs on every one of them


def all_distances(seqs, ref):
    """mbr_ref.edit_distance of every sequence against ref.  The (20, 8, 8) lattices have 10^5 distinct paths and the plain
    Python DP would take a minute per lattice, so beyond PLAIN_LIMIT sequences the same unit-cost recurrence runs for all
    of them at once in numpy (rows = the sequences' labels, the reference along the columns, the chain along a row as a
    prefix minimum), and mbr_ref.edit_distance itself is held against it on the PLAIN_LIMIT smallest distances (the ones
    that decide the minimum) and on as many sequences drawn at random."""
    ref = [int(x) for x in ref]
    if len(seqs) <= PLAIN_LIMIT:
        return np.asarray([R.edit_distance(s, ref) for s in seqs], np.int64)
    n, m = len(seqs), max(len(s) for s in seqs)
    x = np.zeros((n, m), np.int64)
    lens = np.asarray([len(s) for s in seqs])
    for i, s in enumerate(seqs):
        x[i, :len(s)] = s
    j, y = np.arange(len(ref) + 1), np.asarray(ref, np.int64)
    row = np.tile(j, (n, 1))
    out = np.where(lens == 0, len(ref), -1)
    for i in range(1, m + 1):
        t = np.concatenate([np.full((n, 1), i), np.minimum(row[:, 1:] + 1, row[:, :-1] + (x[:, i - 1:i] != y[None, :]))], axis=1)
        row = np.minimum.accumulate(t - j, axis=1) + j
        out = np.where(lens == i, row[:, -1], out)
    pick = np.concatenate([np.argsort(out, kind="stable")[:PLAIN_LIMIT], np.random.default_rng(0).integers(0, n, PLAIN_LIMIT)])
    for i in pick:
        assert R.edit_distance(seqs[i], ref) == out[i]
    return out


_PATHS = {}


def every_path(P, lab):
    key = (id(P), lab.tobytes())
    if key not in _PATHS:
        ps = O.paths(P, lab)
        _PATHS[key] = (P, {(tuple(a), tuple(w)) for a, w in ps}, sorted({tuple(w) for _, w in ps}))
    return _PATHS[key][1:]


def check(P, ref, skip_words=()):
    """oracle_ref on (P, ref) against the enumeration; returns the record."""
    lab, r = O.labels(P, skip_words), O.local_ref(P, ref)
    D = O.table(P, lab, r)
    out = O.backtrace(P, lab, r, D)
    every, seqs = every_path(P, lab)
    assert out["errors"] == all_distances(seqs, r).min()
    assert (tuple(out["arcs"]), tuple(out["words"])) in every
    assert R.edit_distance(out["words"], list(r)) == out["errors"] == out["ins"] + out["dele"] + out["sub"]
    assert D.dtype == np.int64 and (D[0] == np.arange(r.size + 1)).all() and (np.diff(D, axis=1) <= 1).all()
    return out


@pytest.mark.parametrize("shape", R.SHAPES[:5])
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_against_the_enumeration_of_all_paths(shape, seed):
    P = score.pack_lattice(R.random_lattice(*shape, seed=seed))
    rng = np.random.default_rng(100 + seed)
    for n in (0, 1, P.depth, P.depth + 3):
        ref = rng.integers(1, shape[2] + 2, n)              # 1 .. vocab + 1: some words are not in the lattice
        check(P, ref)


def test_reference_word_outside_the_lattice_never_matches():
    P = score.pack_lattice(R.paths_lattice([([3, 4], 0.5), ([3, 5], 0.5)]))
    assert O.local_ref(P, [3, 9, 4]).tolist() == [1, -1, 2]
    out = check(P, [3, 9])
    assert out["errors"] == 1 and out["sub"] == 1


def test_skipped_words_are_free_and_never_match():
    lat = R.paths_lattice([([3, 7, 4], 0.5), ([3, 5], 0.5)])
    P = score.pack_lattice(lat)
    plain, skipped = check(P, [3, 4]), check(P, [3, 4], skip_words=(7,))
    assert plain["errors"] == 1 and skipped["errors"] == 0
    assert [int(P.word_ids[w]) for w in skipped["words"]] == [3, 4] and len(skipped["arcs"]) == 4    # 3 word arcs + the final
    # a reference word in the skip set never matches: the arc of 7 is free, the reference's 7 is a deletion
    both = check(P, [3, 7, 4], skip_words=(7,))
    assert both["errors"] == 1 and both["dele"] == 1 and check(P, [3, 7, 4])["errors"] == 0
    assert (O.labels(P, ()) == P.word).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_linear_lattice_equals_edit_distance(seed):
    rng = np.random.default_rng(seed)
    hyp = [int(w) for w in rng.integers(1, 6, int(rng.integers(1, 12)))]
    ref = [int(w) for w in rng.integers(1, 7, int(rng.integers(0, 12)))]
    P = score.pack_lattice(R.paths_lattice([(hyp, 1.0)]))
    out = O.oracle(P, ref)
    assert out["errors"] == R.edit_distance(hyp, ref) and out["words"] == hyp
    assert out["arcs"] == list(range(len(hyp))) and len(out["packed_arcs"]) == len(hyp) + 1


def test_tie_rule_arc_order_first_then_diagonal_free_insertion():
    # two arcs with the same cost: the lower packed index wins
    P = score.pack_lattice(R.paths_lattice([([5], 0.5), ([6], 0.5)]))
    out = O.oracle(P, [7])
    assert out["errors"] == 1 and out["words"] == [5] and out["sub"] == 1
    # [b] against [a b]: the diagonal is tried first, so b matches and a is deleted
    out = O.oracle(score.pack_lattice(R.paths_lattice([([2], 1.0)])), [1, 2])
    assert (out["errors"], out["ins"], out["dele"], out["sub"]) == (1, 0, 1, 0)
    # [a b] against [b]: the insertion of a and the match of b (not a substitution and an insertion)
    out = O.oracle(score.pack_lattice(R.paths_lattice([([1, 2], 1.0)])), [2])
    assert (out["errors"], out["ins"], out["dele"], out["sub"]) == (1, 1, 0, 0)
    # [a] against [b c]: cost 2 as substitution + deletion; the walk tries the arc (diagonal) before the deletion
    out = O.oracle(score.pack_lattice(R.paths_lattice([([1], 1.0)])), [2, 3])
    assert (out["errors"], out["ins"], out["dele"], out["sub"]) == (2, 0, 1, 1)


def test_lattice_depth_on_known_strings():
    lat = {k: v for k, v in R.paths_lattice([([1, 2], 0.6), ([1, 3], 0.4)]).items() if k != "tid"}
    arc_len, final_len = [4, 6, 5, 5], [0, 0, 2, 0, 2]
    lat["tid_off"] = np.concatenate([[0], np.cumsum(arc_len)]).astype(np.int64)
    lat["tids"] = np.ones(int(np.sum(arc_len)), np.int32)
    lat["final_acoustic"] = np.zeros(5, np.float32)
    lat["final_tid_off"] = np.concatenate([[0], np.cumsum(final_len)]).astype(np.int64)
    lat["final_tids"] = np.ones(int(np.sum(final_len)), np.int32)
    P = score.pack_lattice(lat)
    assert score.lattice_depth(P) == (4 + 6 + 5 + 5 + 2 + 2, 12)          # two paths of 12 frames: depth 2
    bare = score.pack_lattice({k: v for k, v in R.paths_lattice([([1], 1.0)]).items() if k != "tid"})
    assert score.lattice_depth(bare) is None
    recs = [dict(errors=2), dict(errors=1)]
    assert score.oracle_wer(recs, [[1, 2, 3], [4]]) == (3, 4)
