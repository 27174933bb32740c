"""The CPU side of the large-graph cases (tests/graph_cases.py) the GPU tests of the Viterbi and the alignment-free
numerator lean on: every rung lands on the route it is meant to pin, the binding beams bind without losing every final
state, the tie case meets ties, and the oracle stays finite on the scale-range logits.  No GPU needed; the references
computed here are the ones the GPU tests reuse in the same process."""
import numpy as np
import pytest

import graph_cases as GC
import num_graph_ref as R


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_rung_routes_and_binding_beam(k):
    g = GC.rung_graph(k)                    # asserts the state range and the states per thread of the rung
    S, A = g["final"].shape[0], g["src"].shape[0]
    vit, chains, post = GC.viterbi_lds(S, A), GC.chains_lds(S, A), GC.post_lds(S)
    print("rung %d: S %d A %d T %d LDS viterbi %d ng_chains %d ng_post %d" % (k, S, A, GC.rung(k)[1], vit, chains, post))
    if k == 1:
        assert vit <= GC.LDS_OPT_IN < chains <= GC.LDS_LIMIT
        assert S > 3 * GC.THREADS               # a third and a fourth state per lane: beyond the numerator's prefetch
    elif k == 2:
        assert GC.LDS_OPT_IN < vit <= GC.LDS_LIMIT and GC.LDS_LIMIT - 16 * 1024 < chains <= GC.LDS_LIMIT
    elif k == 3:
        assert vit > GC.LDS_LIMIT and chains > GC.LDS_LIMIT and post <= GC.LDS_OPT_IN
    else:
        assert vit > GC.LDS_LIMIT and chains > GC.LDS_LIMIT and 8 * S > GC.LDS_OPT_IN
    assert int(np.diff(g["in_off"]).max()) < 65536
    (wide, wtrace), (tight, ttrace) = GC.viterbi_reference(k, 1e30), GC.viterbi_reference(k, GC.BINDING_BEAM[k])
    assert wide[0] == 0 and wtrace["pruned"] == 0
    assert tight[0] == 0 and ttrace["pruned"] > 0
    # the beam is below what the unpruned best path needs, so that path is gone; another one still reaches a final state
    assert GC.BINDING_BEAM[k] < wtrace["margin"]
    assert GC.differs(wide, tight) and float(tight[2]) > float(wide[2])


def test_tie_case_meets_ties():
    graphs, T, beams = GC.ties_case()
    assert graphs.status == [0] and graphs.num_states[0] > 1024
    g = graphs.export(0)
    assert int(np.isfinite(g["final"]).sum()) >= 2
    for beam in beams:
        ref, trace = GC.ties_reference(beam)
        print("beam %g: %s" % (beam, {k: v for k, v in trace.items() if k != "excess"}))
        assert ref[0] == 0
        assert trace["arc_ties"] > 0          # a later in-arc equalled the best so far: strict < kept the earlier one
        assert trace["final_ties"] >= 2       # two final states with the least total: the lowest index wins
    assert GC.ties_reference(beams[-1])[1]["pruned"] > 0 or len(beams) == 1


def test_scale_range_logits_keep_the_oracle_finite():
    for gap in (60.0, 200.0):
        c = GC.scale_range_case(gap)
        lp, gamma = c["want"]
        assert np.isfinite(lp) and np.isfinite(gamma).all() and np.abs(gamma.sum(1) - 1.0).max() <= 1e-9
        for t, q in c["outliers"]:
            assert 0 < t < c["T"] - 1 or t == 0
            assert c["x"][t, q] == np.delete(c["x"][t], q).max() + np.float32(gap)
            assert gamma[t, q] == 0.0           # no arc that is ever taken at frame t carries pdf q
        assert {t for t, _ in c["outliers"]} >= {0} and len(c["outliers"]) == 2
        # the outliers change nothing but the scale of two frames: the posteriors are those of the plain logits
        assert np.abs(gamma - c["plain"][1]).max() <= 1e-12 and abs(lp - c["plain"][0]) <= 1e-9 * abs(lp)
