"""CPU pins of tests/num_cases.py: the generator keeps its invariants and every case still has the frames that put it among
the numerator tests (a later change cannot quietly empty them), the oracle's posteriors are distributions, and the float32
restatement of the kernel's recursion stays inside the bounds the GPU tests use -- which are 4 x its measured error."""
import numpy as np
import pytest

import num_cases as nc

ALL = sorted(nc.CASES)


@pytest.mark.parametrize("name", ALL)
def test_generator_invariants(name):
    c = nc.case(name)
    f = c.fst
    T, off = c.T, f["frame_offsets"]
    assert off[0] == 0 and off[-1] == c.arcs and off.shape[0] == T + 1
    dead, unre = len(f["dead_states"]), len(f["unreachable_states"])
    extra = np.zeros(T, int)
    if name == "dead_ends":
        assert dead == 5 and unre == 4
        st = f["state_time"]
        np.add.at(extra, st[f["dead_states"]] - 1, 2)          # two arcs into each, in the frame before its layer
        np.add.at(extra, st[f["unreachable_states"]], 2)       # two arcs out of each
    else:
        assert dead == 0 and unre == 0
    assert (np.diff(off) == np.asarray(c.widths) + extra).all()
    # arcs of frame t go from layer t to layer t + 1; the layers have the asked-for sizes
    st = f["state_time"]
    frame = np.repeat(np.arange(T), np.diff(off))
    assert (st[f["src"]] == frame).all() and (st[f["dst"]] == frame + 1).all()
    assert f["num_states"] == sum(c.states) + dead + unre and c.states[0] == 1 and st[0] == 0
    # every state is entered and left, but for the initial state, the final ones and the few of dead_ends
    has_in = np.zeros(f["num_states"], bool); has_in[f["dst"]] = True
    has_out = np.zeros(f["num_states"], bool); has_out[f["src"]] = True
    no_in = set(np.flatnonzero(~has_in)) - {0}
    no_out = set(np.flatnonzero(~has_out)) - set(int(s) for s in f["final_states"])
    assert no_in == set(int(s) for s in f["unreachable_states"]) and no_out == set(int(s) for s in f["dead_states"])
    assert (st[f["final_states"]] == T).all() and f["final_states"].shape[0] == c.states[T] == (st == T).sum()
    assert f["weight"].min() >= 0.0 and f["weight"].max() <= 2.0 and (f["weight"].max() > 1.0 or c.arcs < 8)
    assert f["final_weights"].min() >= 0.0 and f["final_weights"].max() <= 2.0
    assert f["pdf"].min() >= 0 and f["pdf"].max() < nc.P


def test_cases_reach_the_branches_they_are_named_for():
    fa = {n: nc.case(n).frame_arcs for n in ALL}
    one = nc.case("one_frame")
    assert one.T == 1 and one.arcs == 3 and one.fst["final_states"].shape[0] == 2
    for n in ("edges", "peaked"):
        assert nc.case(n).arcs == 2898 and nc.is_staged([nc.case(n)])
        for limit in (nc.DPP_ARCS, nc.WAVE, nc.REG_ARCS[64], nc.REG_ARCS[256]):
            assert ((fa[n] <= limit) & (fa[n] > 1)).any() and (fa[n] > limit).any(), (n, limit)
            assert limit + 1 in fa[n] or limit == nc.DPP_ARCS and 17 in fa[n]
        assert nc.case(n).fst["final_states"].shape[0] > 1
    assert nc.case("peaked").logits.max() == 45.0
    assert nc.case("long").T == 602 and nc.case("long_staged").T == 602
    assert not nc.is_staged([nc.case("long")]) and nc.is_staged([nc.case("long_staged")])
    u = nc.case("unstaged")
    assert u.arcs == 7961 and 5 * u.arcs * 4 > nc.STAGE_MAX_LDS and not nc.is_staged([u])
    assert (u.frame_arcs > nc.REG_ARCS[256]).any() and u.T == 41
    assert nc.case("max_states").fst["num_states"] == nc.NUM_MAX_STATES and nc.case("max_states").T == 3
    assert nc.case("too_many_states").fst["num_states"] == nc.NUM_MAX_STATES + 1
    assert (fa["max_states"] > nc.REG_ARCS[256]).all()
    s = fa["edges_small"]
    assert 16 in s and 17 in s and 64 in s and 65 in s and nc.staged_lds_bytes([nc.case("edges_small")]) < 8192
    assert nc.is_staged([nc.case(n) for n in ("one_frame", "narrow", "edges", "peaked", "dead_ends")])
    assert max(nc.case(n).T for n in ALL if not n.startswith("long")) <= 41


@pytest.mark.parametrize("name", ALL)
def test_oracle_rows_are_distributions(name):
    c = nc.case(name)
    lp, post = nc.oracle(name)
    assert np.isfinite(lp) and np.abs(post.sum(1) - 1.0).max() < 1e-10 and post.min() >= 0.0
    f = c.fst
    # arcs through a dead end or out of a never-entered state carry nothing: their pdfs get the other arcs' share only
    if name == "dead_ends":
        bad = np.isin(f["dst"], f["dead_states"]) | np.isin(f["src"], f["unreachable_states"])
        assert bad.sum() == 18
        keep = dict(f)
        for k in ("src", "dst", "pdf", "weight"):
            keep[k] = f[k][~bad]
        frame = np.repeat(np.arange(c.T), np.diff(f["frame_offsets"]))
        ref = nc.R.NumFstRef(f["num_states"], keep["src"], keep["dst"], keep["pdf"], keep["weight"], f["final_states"],
                             f["final_weights"], f["state_time"])
        lp2, post2 = nc.R.num_forward_backward(c.logits.astype(np.float64), ref)
        assert lp2 == lp and (post2 == post).all() and frame.shape[0] == c.arcs


def test_restatement_against_oracle():
    """The constants of num_cases.py are 4 x the largest error over the cases of num_cases.NAMED (rounded up, at most 10 % above),
    every frame sum of every case is positive in float32, and the cases added here stay inside too -- as does the __expf model
    on the staged cases, the only ones the two-wave body runs."""
    worst_post = worst_lp = 0.0
    for name in ALL:
        post, lp, zmin = nc.restatement_errors(name)
        fpost, flp, fz = nc.restatement_errors(name, fast_exp=True)
        staged = nc.is_staged([nc.case(name)])
        print("%-16s posteriors %.3g  lp %.3g  smallest frame sum %.3g   (__expf model: %.3g  %.3g)%s" % (
            name, post, lp, zmin, fpost, flp, "" if staged else "   unstaged"))
        assert zmin > 0.0 and fz > 0.0, name
        assert post < nc.POST_BOUND and lp < nc.LP_BOUND, name
        if staged:
            assert fpost < nc.POST_BOUND and flp < nc.LP_BOUND, name
        if name in nc.NAMED:
            worst_post, worst_lp = max(worst_post, post), max(worst_lp, lp)
    print("largest over the named cases: posteriors %.3g, lp %.3g" % (worst_post, worst_lp))
    assert 4 * worst_post <= nc.POST_BOUND <= 4.4 * worst_post
    assert 4 * worst_lp <= nc.LP_BOUND <= 4.4 * worst_lp


def test_restatement_sees_a_wrong_recursion():
    """What the bounds are for: the weights of half the arcs of one frame (32 of 2898) off by 0.01 is far outside them."""
    c = nc.case("edges")
    lp, post = nc.oracle("edges")
    f = dict(c.fst)
    f["weight"] = c.fst["weight"].copy()
    lo = c.fst["frame_offsets"][3]
    f["weight"][lo:lo + 32] += 1e-2
    lp2, post2, _ = nc.scaled32(c.logits, f)
    assert np.abs(post2 - post).max() > 10 * nc.POST_BOUND and abs(lp2 - lp) > 10 * nc.LP_BOUND * abs(lp)
