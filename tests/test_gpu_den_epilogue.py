"""The batched row epilogue of the persistent denominator kernel (csrc/chain_den_persist2.hip: EPI) against
the float64 C oracle, with the bounds of tests/test_gpu_den_table.py unchanged (log-probability 1e-3 relative, occupancies
1e-4 absolute), once by default and once with PK2_DP2_EPI=0 (read when the graph is created, as PK2_DP2_TABLE is).  The
graphs are the smallest found at which the epilogue's cases occur, and each asserts from the host-side layout that it
does hit its case:
  small         no rank has more than two entries per thread (pspt = 2), direct arcs, at most one per thread
  direct_cap    a thread with kDirect = 2 direct arcs (backward ordering)
  full_rank     rows padded to one slot: one rank owns exactly ONE row, others 2 x 512 -- every entry of every thread in
                use -- and others end inside the first entry (forward) or the second (backward); no direct arc (Rt = R)
  four_entries  more than 3 x 512 rows in a rank: kPSPT entries per thread -- keeps the row-by-row epilogue
  chunks        a table of 1024 entries: more than two table chunks, the streaming form -- keeps the row-by-row epilogue
1, 2 and 7 frames, one sequence and five (more recursions than teams run at once, a team that idles); leaky 1e-4 and 0."""
import numpy as np
import pytest
import torch

from oracle import chain_c
from oracle import chain_ref as R
from pykaldi2_amd import _lib, chain, synth

pytestmark = pytest.mark.gpu

P = 40
LENS = [7, 1, 2, 7, 2]
KPT = 512
_LAYOUT_VARS = ("PK2_DEN_ORDER", "PK2_DP2_TABLE", "PK2_DP2_RES", "PK2_DP2_TCAP", "PK2_DP2_SHARED", "PK2_DP2_ROWARRAYS",
                "PK2_DEN_PERSIST", "PK2_DEN_ESTEP", "PK2_DP2_EPI")


def _skew_graph(n_light, n_heavy, fan, seed=5):
    """`n_light` states entered by ONE arc each (rows of one slot) and `n_heavy` states entered by ~`fan` arcs: the ranks
    that get the heavy rows hold a few rows, the others as many as their slots."""
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


# name: (graph, layout variables, batched epilogue expected by default)
GRAPHS = {
    "small": (lambda: synth.den_graph_arcs(300, 6000, P, seed=300, loop_pdf_differs=True), {}, True),
    "direct_cap": (lambda: _skew_graph(1024, 200, 40), {}, True),
    "full_rank": (lambda: _skew_graph(24000, 20, 1200), {"PK2_DEN_ESTEP": "1"}, True),
    "four_entries": (lambda: _skew_graph(50000, 30, 1600), {"PK2_DEN_ESTEP": "1"}, False),
    "chunks": (lambda: _skew_graph(1024, 200, 40), {"PK2_DP2_TCAP": "1024", "PK2_DP2_SHARED": "0", "PK2_DEN_PERSIST": "2"},
               False),      # (PK2_DEN_PERSIST=2, as tests/test_gpu_chain.py sets it for a forced layout)
}
_cache = {}


def _case(name, leaky):
    """Graph, logits and the oracle's results: computed once, shared by both switches."""
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


def _check_layout(name, G, epi):
    """The case the graph is there for, from the host-side layout."""
    lf, lb = G.debug_persist2(0), G.debug_persist2(1)
    tf, tb = G.debug_persist2_table(0), G.debug_persist2_table(1)
    rows = [np.diff(l["row_begin"]) for l in (lf, lb)]
    grps = [np.diff(l["grp_begin"]) for l in (lf, lb)]
    most = max(int(r.max()) for r in rows + grps)
    per_thread = [int((t["dprob"] != 0).sum(axis=1).max()) for t in (tf, tb)]
    pl = G.plan(len(LENS), max(LENS))
    streams = [l["pieces"] > 0 or l["K"] > 2 for l in (lf, lb)]
    want = [int(epi and GRAPHS[name][2] and not s) for s in streams]
    assert [pl["fwd_epilogue"], pl["bwd_epilogue"]] == want, (pl, want)
    if name == "small":
        assert most <= 2 * KPT and max(per_thread) == 1 and tf["Rt"] < tf["R"] and tb["Rt"] < tb["R"]
    if name == "direct_cap":
        assert most <= 2 * KPT and per_thread[1] == 2 == tb["kDirect"] and not any(streams)
    if name == "full_rank":
        assert int(rows[0].min()) == 1 and int(rows[0].max()) == 2 * KPT == lf["cap"] and lf["estep"] == 1
        # ... and a tail masked inside the first entry (forward) and inside the second (backward)
        assert ((rows[0] > 1) & (rows[0] < KPT)).any() and ((rows[1] > KPT) & (rows[1] < 2 * KPT)).any()
        assert tf["Rt"] == tf["R"] and tb["Rt"] == tb["R"] and per_thread == [0, 0] and not any(streams)
    if name == "four_entries":
        assert most > 3 * KPT and not any(streams)
    if name == "chunks":
        assert all(streams) and lf["K"] > 2


@pytest.mark.parametrize("leaky", [1e-4, 0.0])
@pytest.mark.parametrize("epi", ["default", "0"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_den_forward_backward_with_either_row_epilogue(name, epi, leaky, monkeypatch):
    for var in _LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in GRAPHS[name][1].items():
        monkeypatch.setenv(var, val)
    if epi == "0":
        monkeypatch.setenv("PK2_DP2_EPI", "0")
    g, lg, want = _case(name, leaky)
    G = chain.DenominatorGraph(g, P)
    _check_layout(name, G, epi == "default")
    assert G.kernel_path(len(LENS)) == 2 and G.persist_form(len(LENS)) == 2 and G.kernel_path(1) == 2
    pl = G.plan(len(LENS), max(LENS))
    assert pl["family"] == 1 and pl["form"] == 2, pl
    x = torch.from_numpy(lg).cuda()
    runs = [(LENS, x), ([LENS[0]], x[:1].contiguous())]                 # five sequences, and one
    for ls, xs in runs:
        lp_t, gamma_t = chain.den_forward_backward(G, xs, ls, leaky)
        lp2_t, gamma2_t = chain.den_forward_backward(G, xs, ls, leaky)
        assert torch.equal(lp_t, lp2_t) and torch.equal(gamma_t, gamma2_t)      # the same bits from call to call
        lp, gamma = lp_t.cpu().numpy(), gamma_t.cpu().numpy()
        assert np.isfinite(lp).all() and not _lib.persist_guard_raised()        # (an aborted launch leaves NaN and raises the guard)
        for n, Tn in enumerate(ls):
            want_lp, want_g, chk = want[n]
            assert abs(chk - 1.0) < 1e-3
            err_lp, err_g = abs(lp[n] - want_lp) / abs(want_lp), np.abs(gamma[n, :Tn] - want_g).max()
            print("%s epi=%s leaky=%g N=%d n=%d T=%d: log-prob rel %.2e, occupancy abs %.2e" % (name, epi, leaky, len(ls), n, Tn, err_lp, err_g))
            assert err_lp <= 1e-3, (n, lp[n], want_lp)
            assert err_g < 1e-4, (n, err_g)
            assert not gamma[n, Tn:].any()
