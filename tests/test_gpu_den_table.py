"""The persistent denominator kernel with the table prefix (csrc/chain_internal.h: kDirectDeg) against the
float64 C oracle, with the bounds tests/test_gpu_chain.py applies to the same quantities (log-probability 1e-3 relative,
occupancies 1e-4 absolute), once by default and once with PK2_DP2_TABLE=full.  The two are not asked to agree bit for bit:
a direct arc's product joins its row's sum at another place.  Shapes: the smallest at which the new paths differ -- a table
of less than one 256-entry DMA row, one that ends inside a row, one that fills its last row exactly and one entry more,
virtual states != states (multi_entry); 1, 2 and 7 frames; one sequence, and five (more recursions than teams)."""
import numpy as np
import pytest
import torch

from oracle import chain_c
from oracle import chain_ref as R
from pykaldi2_amd import chain, synth

pytestmark = pytest.mark.gpu

P = 40
LEAKY = 1e-4
# name: (states, arcs, multi_entry_frac, forward table entries, forward Rt)
GRAPHS = {
    "s300": (300, 6000, 0.0, 150, 256),
    "s1100": (1100, 20000, 0.0, 550, 768),
    "s512_full_row": (512, 8000, 0.0, 256, 256),
    "s514_one_more": (514, 8000, 0.0, 257, 512),
    "s1100_multi_entry": (1100, 20000, 0.3, 550, 768),
}
_cache = {}


def _case(name):
    """Graph, initial probabilities, logits and the oracle's results: computed once, shared by both switches."""
    if name not in _cache:
        S, A, multi, _, _ = GRAPHS[name]
        kw = dict(loop_pdf_differs=True)
        if multi:
            kw["multi_entry_frac"] = multi
        g = synth.den_graph_arcs(S, A, P, seed=S, **kw)
        pi = R.initial_probs_ref(g["num_states"], g["src"].astype(np.int64), g["dst"].astype(np.int64),
                                 g["prob"].astype(np.float64), 0)
        lens = [7, 1, 2, 5, 3]
        lg = np.random.default_rng(S).normal(0, 2, size=(len(lens), max(lens), P)).astype(np.float32)
        want = [chain_c.den_fb(g, pi, lg[n, :T], LEAKY, double=True) for n, T in enumerate(lens)]
        _cache[name] = (g, lens, lg, want)
    return _cache[name]


@pytest.mark.parametrize("table", ["default", "full"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_den_forward_backward_with_and_without_the_table_prefix(name, table, monkeypatch):
    for var in ("PK2_DEN_ORDER", "PK2_DP2_TABLE", "PK2_DP2_RES", "PK2_DP2_TCAP", "PK2_DP2_SHARED", "PK2_DP2_ROWARRAYS", "PK2_DEN_PERSIST"):
        monkeypatch.delenv(var, raising=False)
    if table == "full":
        monkeypatch.setenv("PK2_DP2_TABLE", "full")
    g, lens, lg, want = _case(name)
    S, _, multi, want_entries, want_rt = GRAPHS[name]
    G = chain.DenominatorGraph(g, P)
    assert G.kernel_path(len(lens)) == 2 and G.persist_form(len(lens)) == 2 and G.kernel_path(1) == 2
    tf, tb = G.debug_persist2_table(0), G.debug_persist2_table(1)
    if table == "full":
        assert tf["Rt"] == tf["R"] == S and tb["Rt"] == tb["R"] and tf["direct_arcs"] == 0 and tb["direct_arcs"] == 0
    else:
        assert (tf["table_entries"], tf["Rt"], tf["R"]) == (want_entries, want_rt, S) and tf["direct_arcs"] > 0
        assert tb["Rt"] < tb["R"] and tb["direct_arcs"] > 0 and (tb["R"] > S) == bool(multi)
    x = torch.from_numpy(lg).cuda()
    runs = [(lens, chain.den_forward_backward(G, x, lens, LEAKY))]
    runs.append(([lens[0]], chain.den_forward_backward(G, x[:1].contiguous(), [lens[0]], LEAKY)))      # one sequence
    for ls, (lp, gamma) in runs:
        lp, gamma = lp.cpu().numpy(), gamma.cpu().numpy()
        for n, Tn in enumerate(ls):
            want_lp, want_g, chk = want[n]
            assert abs(chk - 1.0) < 1e-3
            err_lp, err_g = abs(lp[n] - want_lp) / abs(want_lp), np.abs(gamma[n, :Tn] - want_g).max()
            print("%s %s N=%d n=%d T=%d: log-prob rel %.2e, occupancy abs %.2e" % (name, table, len(ls), n, Tn, err_lp, err_g))
            assert err_lp <= 1e-3, (n, lp[n], want_lp)
            assert err_g < 1e-4, (n, err_g)
            assert not gamma[n, Tn:].any()
