"""The forward row epilogue with its as-dependent work in front of the row-sum barrier (csrc/chain_den_persist2.hip: EPI == 2,
the default) against the batched form it is derived from (PK2_DP2_EPI=1, 4.1i), both measured against the
float64 C oracle on the same inputs.  Per quantity the new form's error against the oracle may be at most TWICE the old
form's error against the same oracle (room for one extra rounding per row; the committed form keeps the old one's
operations and their order, and measured the same errors -- profiles/den_epilogue2.txt section 5).  The quantities: the
denominator log-probability per sequence (largest relative error of the call), their sum (the denominator term of the
objective) and the occupancies (the gradient with respect to the logits; largest absolute error).  (The numerator does not
run through this kernel's epilogue; the objective's denominator term is what the switch can change.)

Four sequences of 4, 3, 2 and 1 frames in one call: the first frame comes from pi, the last one publishes nothing, the three
ring-word slots wrap at the fourth.  The graphs, each with its case asserted from the graph or the host-side layout:
  chain        synth.den_graph_arcs' chain topology with some self-loops removed (states with and without a peeled loop)
               and every arc entering a few states removed (states without a row); direct arcs
  multi        the same with multi_entry_frac: states entered with two pdfs -- the per-row loop next to the new code
  skew         no direct arc forward (the whole vector is the table), threads with two backward
  skew_t       skew with every arc turned round: threads with 0, 1 and 2 direct arcs in the FORWARD epilogue
  fallback     more than two table chunks: the streaming form, where 2 falls back as 1 does -- bit-equal results
"""
import numpy as np
import pytest
import torch

from oracle import chain_c
from oracle import chain_ref as R
from pykaldi2_amd import _lib, chain, synth

pytestmark = pytest.mark.gpu

P = 40
LENS = [4, 3, 2, 1]
_LAYOUT_VARS = ("PK2_DEN_ORDER", "PK2_DP2_TABLE", "PK2_DP2_RES", "PK2_DP2_TCAP", "PK2_DP2_SHARED", "PK2_DP2_ROWARRAYS",
                "PK2_DEN_PERSIST", "PK2_DEN_ESTEP", "PK2_DP2_EPI")


def _skew_graph(n_light, n_heavy, fan, seed=5):
    """`n_light` states entered by one arc each and `n_heavy` states entered by ~`fan` arcs (tests/test_gpu_den_epilogue.py)."""
    rng = np.random.default_rng(seed)
    S = n_light + n_heavy
    heavy = np.arange(n_light, S)
    src = [rng.choice(heavy, n_light), np.arange(n_light), np.arange(n_light)]
    dst = [np.arange(n_light), rng.choice(heavy, n_light), rng.choice(heavy, n_light)]
    for h in heavy:
        src.append(rng.choice(heavy, fan))
        dst.append(np.full(fan, h))
    src.append(heavy)
    dst.append(heavy)
    key = np.unique(np.concatenate(src).astype(np.int64) * S + np.concatenate(dst))
    src, dst = key // S, key % S
    state_pdf = rng.integers(0, P, size=S)
    w = rng.gamma(1.0, 1.0, size=src.shape[0]) + 1e-3
    prob = w / np.bincount(src, weights=w, minlength=S)[src]
    return dict(num_states=S, start=0, num_pdfs=P, src=src.astype(np.int32), dst=dst.astype(np.int32),
                pdf=state_pdf[dst].astype(np.int32), prob=prob.astype(np.float32))


def _transposed(g):
    """Every arc turned round (pdfs by destination state as before, probabilities normalised per source state again): what
    the backward ordering of `g` does with its direct arcs, the forward ordering does here."""
    S = g["num_states"]
    state_pdf = np.zeros(S, np.int32)
    state_pdf[g["dst"]] = g["pdf"]
    src, dst = g["dst"].copy(), g["src"].copy()
    order = np.lexsort((dst, src))
    src, dst, w = src[order], dst[order], g["prob"].astype(np.float64)[order]
    out = np.bincount(src, weights=w, minlength=S)
    assert (out > 0).all()
    return dict(num_states=S, start=0, num_pdfs=P, src=src, dst=dst, pdf=state_pdf[dst], prob=(w / out[src]).astype(np.float32))


def _chain_graph(multi):
    """The chain topology of synth.den_graph_arcs (states 2k: entry, 2k + 1: exit of phone k), thinned: the entry states of
    phones 2, 12, 22, ... lose their self-loop, those of phones 5, 15, 25, ... every arc that enters them from another
    state.  The probabilities are normalised per source state again."""
    g = synth.den_graph_arcs(300, 6000, P, seed=300, loop_pdf_differs=True, multi_entry_frac=0.3 if multi else 0.0)
    S = g["num_states"]
    no_loop = np.arange(2, S // 2, 10) * 2
    no_row = np.arange(5, S // 2, 10) * 2
    src, dst = g["src"], g["dst"]
    drop = ((src == dst) & np.isin(src, no_loop)) | ((src != dst) & np.isin(dst, no_row))
    keep = ~drop
    src, dst, pdf, prob = src[keep], dst[keep], g["pdf"][keep], g["prob"][keep].astype(np.float64)
    out = np.bincount(src, weights=prob, minlength=S)
    assert (out > 0).all()                                    # every state still has an arc to leave by
    loops = np.zeros(S, bool)
    loops[src[src == dst]] = True
    entered = np.zeros(S, bool)
    entered[dst[src != dst]] = True
    assert not loops[no_loop].any() and loops.sum() == S - len(no_loop)       # states with and without a peeled self-loop
    assert not entered[no_row].any() and entered.sum() == S - len(no_row)     # states without a row
    if multi:       # a state entered (from other states) with two pdfs: two rows
        key = np.unique(dst[src != dst].astype(np.int64) * P + pdf[src != dst])
        assert (np.bincount(key // P, minlength=S) >= 2).any()
    return dict(num_states=S, start=0, num_pdfs=P, src=src, dst=dst, pdf=pdf, prob=(prob / out[src]).astype(np.float32))


# name: (graph, layout variables, the forward epilogue with PK2_DP2_EPI unset or 2)
GRAPHS = {
    "chain": (lambda: _chain_graph(False), {}, 2),
    "multi": (lambda: _chain_graph(True), {}, 2),
    "skew": (lambda: _skew_graph(1024, 200, 40), {}, 2),
    "skew_t": (lambda: _transposed(_skew_graph(1024, 200, 40)), {}, 2),
    "fallback": (lambda: _skew_graph(1024, 200, 40), {"PK2_DP2_TCAP": "1024", "PK2_DP2_SHARED": "0", "PK2_DEN_PERSIST": "2"}, 0),
}
_cache = {}


def _case(name, leaky):
    if name not in _cache:
        g = GRAPHS[name][0]()
        pi = R.initial_probs_ref(g["num_states"], g["src"].astype(np.int64), g["dst"].astype(np.int64),
                                 g["prob"].astype(np.float64), 0)
        lg = np.random.default_rng(len(name)).normal(0, 2, size=(len(LENS), max(LENS), P)).astype(np.float32)
        _cache[name] = (g, pi, lg, {})
    g, pi, lg, want = _cache[name]
    if leaky not in want:
        want[leaky] = [chain_c.den_fb(g, pi, lg[n, :T], leaky, double=True) for n, T in enumerate(LENS)]
    return g, lg, want[leaky]


def _run(g, lg, epi, monkeypatch):
    """(log-probabilities, occupancies, forward epilogue form, direct arcs per thread [forward, backward]) with PK2_DP2_EPI
    = `epi` (None: unset) when the graph is created."""
    if epi is None:
        monkeypatch.delenv("PK2_DP2_EPI", raising=False)
    else:
        monkeypatch.setenv("PK2_DP2_EPI", epi)
    G = chain.DenominatorGraph(g, P)
    form = int(_lib.lib().pk2_den_graph_persist2_epilogue(G._h, 2))
    per_thread = [np.unique((G.debug_persist2_table(w)["dprob"] != 0).sum(axis=1)).tolist() for w in (0, 1)]
    pl = G.plan(len(LENS), max(LENS))
    assert pl["family"] == 1 and pl["form"] == 2, pl
    assert pl["fwd_epilogue"] == (1 if form else 0)
    lp_t, gamma_t = chain.den_forward_backward(G, torch.from_numpy(lg).cuda(), LENS, 1e-4)
    lp, gamma = lp_t.cpu().numpy().astype(np.float64), gamma_t.cpu().numpy().astype(np.float64)
    assert np.isfinite(lp).all() and not _lib.persist_guard_raised()
    return lp, gamma, form, per_thread


def _errors(lp, gamma, want):
    """[largest relative error of a sequence's log-probability, relative error of their sum, largest absolute error of an
    occupancy] against the oracle."""
    want_lp = np.array([w[0] for w in want], np.float64)
    e_lp = float(np.max(np.abs(lp - want_lp) / np.abs(want_lp)))
    e_obj = float(abs(lp.sum() - want_lp.sum()) / abs(want_lp.sum()))
    e_g = max(float(np.abs(gamma[n, :T] - want[n][1].astype(np.float64)).max()) for n, T in enumerate(LENS))
    for n, T in enumerate(LENS):
        assert abs(want[n][2] - 1.0) < 1e-3 and not gamma[n, T:].any()
    return [e_lp, e_obj, e_g]


@pytest.mark.parametrize("name", ["chain", "multi", "skew", "skew_t"])
def test_new_forward_epilogue_errs_at_most_twice_the_batched_one(name, monkeypatch):
    for var in _LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in GRAPHS[name][1].items():
        monkeypatch.setenv(var, val)
    g, lg, want = _case(name, 1e-4)
    lp1, g1, form1, _ = _run(g, lg, "1", monkeypatch)
    lp2, g2, form2, per_thread = _run(g, lg, "2", monkeypatch)
    lpd, gd, formd, _ = _run(g, lg, None, monkeypatch)
    assert (form1, form2, formd) == (1, 2, 2), (form1, form2, formd)
    assert np.array_equal(lpd, lp2) and np.array_equal(gd, g2)            # unset is 2
    print("%s: direct arcs per thread forward %s backward %s" % (name, per_thread[0], per_thread[1]))
    if name == "skew":
        assert per_thread == [[0], [0, 1, 2]]          # no direct arc forward (the whole vector is the table), two backward
    elif name == "skew_t":
        assert per_thread[0] == [0, 1, 2]              # threads with 0, 1 and 2 direct arcs in the forward epilogue
    else:
        assert per_thread[0] == [0, 1]
    e1, e2 = _errors(lp1, g1, want), _errors(lp2, g2, want)
    for what, a, b in zip(("den_logprob", "objective", "gradient"), e1, e2):
        print("%s %s: error against the oracle, PK2_DP2_EPI=1 %.3e, =2 %.3e" % (name, what, a, b))
    for what, a, b in zip(("den_logprob", "objective", "gradient"), e1, e2):
        assert b <= 2.0 * a, (name, what, a, b)


def test_fallback_is_bit_equal(monkeypatch):
    for var in _LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in GRAPHS["fallback"][1].items():
        monkeypatch.setenv(var, val)
    g, lg, want = _case("fallback", 1e-4)
    lp1, g1, form1, _ = _run(g, lg, "1", monkeypatch)
    lp2, g2, form2, _ = _run(g, lg, "2", monkeypatch)
    assert (form1, form2) == (0, 0)                                       # streamed pieces: the row-by-row form either way
    assert np.array_equal(lp1, lp2) and np.array_equal(g1, g2)
    e = _errors(lp2, g2, want)
    assert e[0] <= 1e-3 and e[2] < 1e-4, e
