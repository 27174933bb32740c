"""MBR system combination on the host: the rule the kernels implement (combine_ref.combine: per-system
E-steps and a weighted reduction) against minimum Bayes risk decoding of the explicit union lattice
(combine_ref.union_mbr), and the host packing of pykaldi2_amd.score (pack_groups: union vocabularies, maps, weights).

The two restatements sum the same products in other orders: risk and confidences are sums of at most A (Q + 1) <= 1e5
products of magnitude <= Q with a few 2^-53 relative error each, so 1e-10 leaves two orders of room (measured when the
rule was fixed: 2.7e-14).  Words and iteration counts must be equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import combine_ref as CR  # noqa: E402
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import score  # noqa: E402

WORST = {}


@pytest.mark.parametrize("seed", range(40))
def test_the_rule_agrees_with_mbr_decoding_of_the_explicit_union(seed):
    lats, weights = CR.case(seed)
    Ps = [score.pack_lattice(lat) for lat in lats]
    for st in R.SETTINGS:
        a, b = CR.combine(Ps, weights, st), CR.union_mbr(Ps, weights, st)
        assert a["words"] == b["words"] and a["iterations"] == b["iterations"] and a["status"] == b["status"] == 0
        err = max([abs(a["risk"] - b["risk"])] + list(np.abs(a["conf"] - b["conf"])))
        WORST["err"] = max(WORST.get("err", 0.0), err)
        WORST["iterations"] = max(WORST.get("iterations", 0), a["iterations"])
        assert err <= 1e-10
        # the first hypothesis is the union's best path
        zs = [R.posteriors(P, st) for P in Ps]
        assert zs[a["system"]]["words"] == b["post"]["words"] or a["margins"]["best_path"] < 1e-9
    print("largest |risk, conf difference| and most E-steps so far:", WORST)


def test_pack_groups_vocabularies_maps_and_weights():
    lats, _ = CR.case(3)
    Ps = [score.pack_lattice(lat) for lat in lats]
    extra = score.pack_lattice(R.paths_lattice([([50, 60], 0.5), ([2, 61], 0.5)]))
    groups, weights = [Ps, [Ps[0], extra], [extra]], [[0.5, 1.5, 2.0][:len(Ps)], [3.0, 1.0], [7.0]]
    H = score.pack_groups(groups, weights)
    flat = [p for g in groups for p in g]
    assert H["group_off"].tolist() == [0, len(Ps), len(Ps) + 2, len(Ps) + 3] and H["group_off"].dtype == np.int32
    assert H["uvoc_off"].dtype == np.int64 and H["uvoc"].dtype == np.int32 and H["map"].dtype == np.int32
    l = 0
    for gi, g in enumerate(groups):
        u = H["uvoc"][H["uvoc_off"][gi]:H["uvoc_off"][gi + 1]]
        assert u[0] == 0 and (np.diff(u) > 0).all() and set(u.tolist()) == set(np.concatenate([p.word_ids for p in g]).tolist())
        assert np.array_equal(u, H["vocab"][gi])
        assert H["cap"][gi] == min(score.MAX_POSITIONS, 2 * max(p.depth for p in g) + 1)
        wn = H["wn"][l:l + len(g)]
        assert abs(wn.sum() - 1.0) <= 1e-15 and np.allclose(wn, np.asarray(weights[gi]) / np.sum(weights[gi]), rtol=1e-15, atol=0)
        assert np.array_equal(H["log_wn"][l:l + len(g)], np.log(wn))
        for p in g:
            m = H["maps"][l]
            assert m.size == u.size and m[0] == 0 and ((m >= 0) & (m <= p.W)).all()
            have = m < p.W
            assert np.array_equal(p.word_ids[m[have]], u[have]) and int(have.sum()) == p.W
            assert not np.isin(u[~have], p.word_ids).any()
            l += 1
    assert np.array_equal(H["map"], np.concatenate(H["maps"])) and l == len(flat)
    assert H["wn"][-1] == 1.0 and H["log_wn"][-1] == 0.0          # a group of one system: weight exactly 1


def test_pack_groups_refusals():
    P = score.pack_lattice(R.paths_lattice([([1, 2], 1.0)]))
    for ws in ([1.0, 2.0], [0.0], [-1.0], [float("inf")], [float("nan")]):
        with pytest.raises(ValueError):
            score.pack_groups([[P]], [ws])
    with pytest.raises(ValueError):
        score.pack_groups([[P] * 9], [[1.0] * 9])
    with pytest.raises(ValueError):
        score.pack_groups([[]], [[]])
