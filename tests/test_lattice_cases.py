"""CPU pins of tests/lattice_cases.py: every wide case still has the frames that put it among the forward-backward tests
(a later change to synth cannot quietly empty them), the float32 accumulation model alone stays inside the posterior
bound it produces, and the dynamic-range lattice keeps both branches with the totals the GPU tests rely on."""
import math

import numpy as np
import pytest

import lattice_cases as lc
import ts_ref
from oracle import lattice_ref as lr


def test_wide_a_runs_both_overflow_loops():
    c = lc.wide("WIDE_A")
    tok, em, ep = lc.frame_counts(c.A, c.T)
    assert ((em > lc.LIN_EMIT_SLOTS) & (tok <= lc.LDS_FRAME_TOKENS)).any(), (tok, em)
    assert (ep > lc.LIN_EPS_SLOTS).any(), ep
    assert tok.max() <= lc.LDS_FRAME_TOKENS          # every frame in LDS: the overflow loops run on the linear path


def test_wide_b_backward_recursion_starts_on_an_epsilon_overflow():
    c = lc.wide("WIDE_B")
    tok, em, ep = lc.frame_counts(c.A, c.T)
    assert ep[c.T] > lc.LIN_EPS_SLOTS, ep
    assert tok.max() <= lc.LDS_FRAME_TOKENS


def test_wide_c_crosses_between_lds_and_global_memory_frames():
    c = lc.wide("WIDE_C")
    tok, em, ep = lc.frame_counts(c.A, c.T)
    above = np.flatnonzero(tok > lc.LDS_FRAME_TOKENS)
    assert (tok <= lc.LDS_FRAME_TOKENS).any() and above.size, tok
    assert above[0] > 0, tok                          # the forward pass is linear before it turns to logs


def test_wide_d_fills_the_register_slots_without_the_overflow_loop():
    c = lc.wide("WIDE_D")
    tok, em, ep = lc.frame_counts(c.A, c.T)
    assert ((em > 3 * lc.LIN_THREADS) & (em <= lc.LIN_EMIT_SLOTS)).any(), em
    assert em.max() <= lc.LIN_EMIT_SLOTS and ep.max() <= lc.LIN_EPS_SLOTS


ALL_CASES = sorted(lc.WIDE) + ["CASES0", "CASES1", "CASES2", "RANGE_120", "RANGE_300", "RANGE_600", "RANGE_1200"]


@pytest.mark.parametrize("name", ALL_CASES)
def test_float32_model_stays_inside_its_bound(name):
    """Every case and setting the GPU tests run: the bound is 4 x the model's deviation over orders drawn with seed 0, so other
    draws of the same model must fit; and the per-link terms are the oracle's -- summed in float64 they give its matrix."""
    c = lc.case(name)
    t2p = c.tm["tid2pdf"]
    for criterion, args in lc.settings(name):
        if criterion == "mmi":
            terms, scale = lc.terms_mmi(c.want, c.ali, t2p, 1.0, args[0], args[1]), 1.0
            want = lr.lattice_mmi(c.want, c.ali, t2p, c.P, 1.0, args[0], args[1])[1]
        elif criterion == "posteriors":
            terms, scale = lc.terms_posteriors(c.want, t2p, 1.0, args[0]), 1.0
            want = ts_ref.posteriors(dict(c.A, start_tok=c.want.start_tok, T=c.T), t2p, c.P, 1.0, args[0])[1]
        else:
            terms = lc.terms_mpe(c.want, c.ali, c.tm, c.P, args[0], args[1])
            want = lr.lattice_mpe(c.want, c.ali, t2p, c.tm["tid2phone"], c.tm["silence_phones"], c.P, args[0], args[1])[1]
            scale = max(1.0, np.abs(want).max())
        t, pdf, val = terms
        mat = np.zeros((c.T, c.P))
        np.add.at(mat, (t, pdf), val)
        assert np.abs(mat - want).max() < 1e-12 * scale, (criterion, args)
        bound = lc.post_bound(t, pdf, val, c.T, c.P, scale)
        other = lc.f32_model_deviation(t, pdf, val, c.T, c.P, orders=8, seed=1) * scale
        print("%s %s %s: bound %.3g, float32 model on fresh orders %.3g, most terms in a cell %d" % (
            name, criterion, args, bound, other, np.bincount(t * c.P + pdf).max()))
        assert other < bound, (criterion, args)


@pytest.mark.parametrize("Xh", [120, 300, 600, 1200])
def test_range_lattice_keeps_both_branches(Xh):
    c = lc.range_case(Xh / lc.RANGE_H)
    a, b = c.branch_pdfs
    pdfs = set(int(c.tm["tid2pdf"][t]) for t in c.A["link_tid"] if t > 0)
    assert pdfs & set(a) and pdfs & set(b) and pdfs <= set(a) | set(b)
    fin = c.A["tok_final"][c.A["tok_frame"] == c.T]
    assert (fin != lr.INF).sum() == 2                 # each branch reaches its own final state
    tot, alpha, beta, like, order, A = lr.lattice_forward_backward(c.want, 1.0, 1.0)
    # B pays X in each of the first h frames and nothing after (A: 2 X in each of the T - h last ones); the graph costs of
    # a path (~10) and the log of the number of B's paths (C(23, 7): 12.4) nearly cancel
    assert abs(tot + Xh) < 20.0
    t, pdf, g = lc.terms_posteriors(c.want, c.tm["tid2pdf"], 1.0, 1.0)
    in_b = np.isin(pdf, b)
    per_frame_b = np.bincount(t[in_b], weights=g[in_b], minlength=c.T)
    assert np.abs(per_frame_b - 1.0).max() < 1e-9     # B's posterior is 1 (A's is exp(-X h)) on every frame
    assert math.isfinite(tot)
