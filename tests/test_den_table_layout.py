"""Table prefix of the persistent denominator layout (csrc/chain_internal.h: kDirectDeg / kDirect), host side
only: an entry of the state vector that a single arc reads stays out of the LDS table -- the published vector has a position
order of its own (table entries first), only [0, Rt) is copied, and the arcs that gather beyond Rt are direct arcs of the
thread that owns their row in the row epilogue.  The numpy model of a frame is tests/test_abi.py's, run over the prefix alone (whatever lies at or
beyond Rt is NaN in the modelled LDS) plus the direct arcs taken from the full vector; the bound is the one
test_den_graph_persistent2_layouts uses."""
import numpy as np
import pytest

from pykaldi2_amd import chain, synth
from test_abi import _emulate_persist2

P = 23


def _graph_views(g, G):
    of = G.debug_ordering(3)
    voff, vpdf = of["voff"], of["vpdf"]
    S = g["num_states"]
    return dict(S=S, V=len(vpdf), vpdf=vpdf, lpdf=of["loop_pdf"], lprob=of["loop_prob"].astype(np.float64),
                vstate=np.repeat(np.arange(S), np.diff(voff)))


def _frame_rows(G, which, vec):
    """Row sums of one frame of ordering `which` over the vector `vec` (caller's entry order): the resident passes over the
    table prefix at the entries' positions, then the direct arcs."""
    lay, tab = G.debug_persist2(which), G.debug_persist2_table(which)
    Rt, R = tab["Rt"], tab["R"]
    assert lay["R"] == R == len(vec) and lay["cbeg"][lay["K"]] == Rt
    assert sorted(tab["pos"]) == list(range(R))                       # a permutation of the vector
    published = np.empty(R)
    published[tab["pos"]] = vec
    rows = _emulate_persist2(dict(lay, R=Rt), published[:Rt])           # (the model's LDS holds NaN wherever no chunk was copied)
    row0 = lay["row_begin"][:-1].astype(np.int64)[:, None, None]
    live = tab["dprob"] != 0
    np.add.at(rows, (row0 + tab["drow"])[live], (tab["dprob"].astype(np.float64) * published[tab["dpos"]])[live])
    return rows, lay, tab


def _check_prefix_invariants(lay, tab):
    Rt = tab["Rt"]
    # every slot of the resident passes -- arcs and null slots alike -- gathers below Rt
    offs = np.concatenate([lay["idx2"] & 0xffff, lay["idx2"] >> 16]).astype(np.int64)
    assert lay["K"] == 2 and lay["pieces"] == 0 and lay["lds_off"][1] == lay["cbeg"][1]
    assert offs.max() < Rt
    assert tab["dprob"].shape[1] == tab["kDirect"] == 2               # at most kDirect records per thread, by construction ...
    live = tab["dprob"] != 0
    assert live.sum(axis=(1, 2)).max() == tab["max_direct"] <= tab["kDirect"] * lay["T"]
    assert live.sum() == tab["direct_arcs"]
    assert (tab["dpos"][live] >= Rt).all() and (tab["dpos"][~live] == 0).all()     # ... direct arcs read beyond the table only
    nrows = np.diff(lay["row_begin"]).astype(np.int64)[:, None, None]
    assert (tab["drow"] < nrows)[live].all() and (tab["drow"][~live] == 0xffff).all()
    # a direct arc sits with the thread that owns its row in the row epilogue: a thread per state forward (whole groups
    # of rows), a thread per row backward -- local index modulo the workgroup's threads
    r, _, tid = np.nonzero(live)
    row = lay["row_begin"][r] + tab["drow"][live]
    if "group_of_row" in tab:
        assert ((tab["group_of_row"][row] - lay["grp_begin"][r]) % lay["T"] == tid).all()
    else:
        assert ((row - lay["row_begin"][r]) % lay["T"] == tid).all()


def _check_sums(g, G, want_prefix=(True, True)):
    v = _graph_views(g, G)
    S, vstate = v["S"], v["vstate"]
    rng = np.random.default_rng(1)
    al, be, x = rng.random(S), rng.random(S), rng.random(g["num_pdfs"])
    xv = np.where(v["vpdf"] >= 0, x[np.maximum(v["vpdf"], 0)], 1.0)
    xl = np.where(v["lpdf"] >= 0, x[np.maximum(v["lpdf"], 0)], 1.0)
    src, dst, pdf, prob = g["src"], g["dst"], g["pdf"], g["prob"].astype(np.float64)
    out = []
    for which, vec in ((0, al), (1, be[vstate] * xv)):
        rows, lay, tab = _frame_rows(G, which, vec)
        if which == 0:
            tab["group_of_row"] = vstate
        if want_prefix[which]:
            assert tab["Rt"] < tab["R"] and tab["Rt"] % 256 == 0, (which, tab["Rt"], tab["R"])
            _check_prefix_invariants(lay, tab)
        if which == 0:
            got = np.bincount(vstate, weights=rows * xv, minlength=S) + al * v["lprob"] * xl
            want = np.bincount(dst, weights=al[src] * prob * x[pdf], minlength=S)
        else:
            got = rows + v["lprob"] * xl * be
            want = np.bincount(src, weights=be[dst] * prob * x[pdf], minlength=S)
        assert np.abs(got - want).max() < 1e-9 * max(1.0, np.abs(want).max()), which
        out.append((lay, tab))
    return out


@pytest.mark.parametrize("multi", [0.0, 0.3])
def test_two_state_phones_leave_half_of_the_vector_out(multi, monkeypatch):
    for name in ("PK2_DEN_ORDER", "PK2_DP2_TABLE", "PK2_DP2_RES", "PK2_DP2_TCAP", "PK2_DP2_SHARED", "PK2_DP2_ROWARRAYS"):
        monkeypatch.delenv(name, raising=False)
    kw = dict(loop_pdf_differs=True)
    if multi:
        kw["multi_entry_frac"] = multi
    g = synth.den_graph_arcs(300, 6000, P, 7, **kw)
    G = chain.DenominatorGraph(g, P)
    (lf, tf), (lb, tb) = _check_sums(g, G)
    if not multi:       # the entry states' alpha and the exit states' virtual states are read once: a property of the graph
        assert (tf["table_entries"], tb["table_entries"]) == (150, 145)
    pl = G.plan(2, 50)
    assert pl["fwd_table"] == (tf["Rt"], tf["R"]) and pl["bwd_table"] == (tb["Rt"], tb["R"])
    assert pl["fwd_direct_arcs"] == tf["direct_arcs"] > 0 and pl["bwd_direct_arcs"] == tb["direct_arcs"] > 0
    # the switch: the whole vector, the layout of an explicit state order (which tests/test_abi.py pins)
    monkeypatch.setenv("PK2_DP2_TABLE", "full")
    G2 = chain.DenominatorGraph(g, P)
    for which in (0, 1):
        t2 = G2.debug_persist2_table(which)
        assert t2["Rt"] == t2["R"] and t2["direct_arcs"] == 0 and (t2["pos"] == np.arange(t2["R"])).all()


def _dense_graph(S=300, fan=4, seed=3):
    """Every state has `fan` non-loop arcs out and in (dst = src + stride) and a self-loop: no entry is read by fewer."""
    rng = np.random.default_rng(seed)
    strides = [1, 7, 31, 101][:fan]
    s = np.arange(S)
    src = np.concatenate([s] + [s for _ in strides])
    dst = np.concatenate([s] + [(s + k) % S for k in strides])
    state_pdf = rng.integers(0, P, size=S)
    w = rng.gamma(1.0, 1.0, size=src.shape[0]) + 1e-3
    prob = w / np.bincount(src, weights=w, minlength=S)[src]
    order = np.lexsort((dst, src))
    return dict(num_states=S, start=0, num_pdfs=P, src=src[order].astype(np.int32), dst=dst[order].astype(np.int32),
                pdf=state_pdf[dst][order].astype(np.int32), prob=prob[order].astype(np.float32))


def test_a_graph_with_nothing_to_leave_out_keeps_its_layout(monkeypatch):
    for name in ("PK2_DEN_ORDER", "PK2_DP2_TABLE"):
        monkeypatch.delenv(name, raising=False)
    g = _dense_graph()
    G = chain.DenominatorGraph(g, P)
    monkeypatch.setenv("PK2_DP2_TABLE", "full")
    G2 = chain.DenominatorGraph(g, P)
    for which in (0, 1):
        tab = G.debug_persist2_table(which)
        assert tab["Rt"] == tab["R"] and tab["direct_arcs"] == 0 and not tab["dprob"].any()
        a, b = G.debug_persist2(which), G2.debug_persist2(which)
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (which, k)
    _check_sums(g, G, want_prefix=(False, False))


@pytest.mark.parametrize("case", ["order_none", "overflow_res8"])
def test_forced_layouts_keep_the_whole_vector(case, monkeypatch):
    monkeypatch.delenv("PK2_DP2_TABLE", raising=False)
    if case == "order_none":
        monkeypatch.setenv("PK2_DEN_ORDER", "none")
        g = synth.den_graph_arcs(300, 6000, P, 7, loop_pdf_differs=True)
    else:
        monkeypatch.delenv("PK2_DEN_ORDER", raising=False)
        monkeypatch.setenv("PK2_DP2_RES", "8")
        g = synth.den_graph_arcs(600, 300000, P, 7, loop_pdf_differs=True, multi_entry_frac=0.2)
    G = chain.DenominatorGraph(g, P)
    for which in (0, 1):
        tab = G.debug_persist2_table(which)
        assert tab["Rt"] == tab["R"] and tab["direct_arcs"] == 0, (case, which)
    if case == "overflow_res8":
        assert G.debug_persist2(0)["pieces"] > 0


def _cap_graph(seed=5):
    """3000 light states (a self-loop and ONE arc out) whose arcs all enter 20 collector states: 150 direct arcs for the thread
    that owns a collector's row, far more than kDirect.  1200 more light states each enter a state of their own (one direct
    arc per row: these stay out of the table), 300 heavy states carry the rest of the graph."""
    rng = np.random.default_rng(seed)
    nl, nc, nh, n2 = 3000, 20, 300, 1200
    S = nl + nc + nh + 2 * n2
    light, coll, heavy = np.arange(nl), nl + np.arange(nc), nl + nc + np.arange(nh)
    light2, mid = nl + nc + nh + np.arange(n2), nl + nc + nh + n2 + np.arange(n2)
    src = [np.arange(S), light, np.repeat(coll, 3), np.repeat(heavy, 400), light2, np.repeat(mid, 3)]
    dst = [np.arange(S), coll[light % nc], rng.choice(heavy, size=3 * nc), rng.choice(nl + nc + nh, size=400 * nh), mid,
           rng.choice(heavy, size=3 * n2)]
    src, dst = np.concatenate(src), np.concatenate(dst)
    # every light state is entered from heavy ones
    for tgt in (light, light2):
        for k in range(3):
            src, dst = np.concatenate([src, heavy[(tgt + k * 7) % nh]]), np.concatenate([dst, tgt])
    state_pdf = rng.integers(0, P, size=S)
    w = rng.gamma(1.0, 1.0, size=src.shape[0]) + 1e-3
    prob = w / np.bincount(src, weights=w, minlength=S)[src]
    order = np.lexsort((dst, src))
    return dict(num_states=S, start=int(heavy[0]), num_pdfs=P, src=src[order].astype(np.int32), dst=dst[order].astype(np.int32),
                pdf=state_pdf[dst][order].astype(np.int32), prob=prob[order].astype(np.float32)), (nl, nc, n2)


def test_a_thread_over_the_cap_takes_entries_back_into_the_table(monkeypatch):
    for name in ("PK2_DEN_ORDER", "PK2_DP2_TABLE"):
        monkeypatch.delenv(name, raising=False)
    g, (nl, nc, n2) = _cap_graph()
    G = chain.DenominatorGraph(g, P)
    (lf, tf), _ = _check_sums(g, G, want_prefix=(True, False))      # (backward: every virtual state is entered by many arcs)
    v = _graph_views(g, G)
    assert v["V"] == v["S"]                                             # (one pdf per destination: a row is a state)
    # without the cap every light state's alpha would stay out of the table and a collector's row would have 150 direct arcs
    read_once = np.bincount(g["src"][g["src"] != g["dst"]], minlength=v["S"]) == 1
    assert read_once.sum() == nl + n2
    live = tf["dprob"] != 0
    assert live.sum(axis=1).max() <= tf["kDirect"] and tf["direct_arcs"] == live.sum()
    # (entries in the slack of the last DMA row, and those of a thread that owns three rows, are table entries as well)
    assert n2 // 2 <= tf["direct_arcs"] <= n2 + tf["kDirect"] * nc
    assert tf["table_entries"] >= v["S"] - n2 - tf["kDirect"] * nc > v["S"] - read_once.sum()


@pytest.fixture(scope="module")
def bench_graph():
    g = synth.den_graph_arcs(30000, 1000000, 6048, 0, loop_pdf_differs=True)
    return g, chain.DenominatorGraph(g, 6048)


def test_bench_graph_halves_its_table(bench_graph, monkeypatch):
    g, G = bench_graph
    for which, want_entries, want_direct in ((0, 15000, 525), (1, 14420, 497)):
        tab = G.debug_persist2_table(which)
        lay = G.debug_persist2(which)
        assert tab["Rt"] <= 0.55 * tab["R"], (which, tab["Rt"], tab["R"])
        assert tab["max_direct"] <= tab["kDirect"] * lay["T"]
        _check_prefix_invariants(lay, tab)
        print("bench graph, direction %d: Rt %d of %d, %d table entries (reference %d), %d direct arcs, %d on the fullest rank "
              "(reference %d)" % (which, tab["Rt"], tab["R"], tab["table_entries"], want_entries, tab["direct_arcs"],
                                  tab["max_direct"], want_direct))
        assert abs(tab["table_entries"] - want_entries) <= 0.02 * want_entries
