"""The alignment-free LF-MMI numerator on the device (csrc/chain_num_graph.hip) and the chain objective over it, against
the float64 oracle of tests/num_graph_ref.py on the same float32 logits.  Tolerances are the chain path's
(tests/test_gpu_chain.py): log-probabilities 1e-3 |want| + 1e-4, posteriors and gradients 1e-4 absolute."""
import numpy as np
import pytest
import torch

from oracle import chain_ref as CR
from pykaldi2_amd import _lib, chain, ops, synth

import graph_cases as GC
import num_graph_ref as R
from test_align_graph import PRONS, kaldi_like_lexicon, make_model
from test_gpu_align import _planted

pytestmark = pytest.mark.gpu

PDFS = 60
PRONS1 = PRONS + [(6, [7], 0.2, None)]      # phone 7 has the one-state chain topology: a word of one frame


def _aligner(N=3, P=1, seed=7, num_pdfs=PDFS):
    tree, tm = make_model(7, N, P, seed=seed, num_pdfs=num_pdfs)
    return chain.MappedAligner.from_models(tm, tree, kaldi_like_lexicon(PRONS1), disambig=[9, 10])


def _min_frames(aligner, words):
    for T in range(1, 400):
        if aligner.compile([words], [T]).status == [chain.ALIGN_OK]:
            return T
    raise AssertionError("no feasible length")


def _poisoned(lls, P, fill=float("nan"), device="cuda"):
    """The utterances' logits inside a larger NaN-filled buffer: both row strides non-trivial, padding is poison."""
    N, Tmax = len(lls), max(ll.shape[0] for ll in lls)
    big = torch.full((N, Tmax + 3, P + 9), fill, dtype=torch.float32, device=device)
    x = big[:, :Tmax, :P]
    for n, ll in enumerate(lls):
        x[n, :ll.shape[0]] = torch.from_numpy(ll).to(device)
    return x


def _check_numerator(gs, lls, x, lp_rel=1e-3, want=None):
    """Stand-alone entry on (gs, x): adds into a pre-filled buffer; every compiled utterance against the oracle
    (want[n]: its result on utterance n when it has been computed before)."""
    fill = 0.25
    grad = torch.full_like(x, fill)
    lp, got = chain.num_graph_forward_backward(gs, x, grad=grad)
    assert got is grad
    lp, got, status = lp.cpu().numpy(), got.cpu().numpy(), lp.status.cpu().numpy()
    assert status.tolist() == gs.status
    for n, ll in enumerate(lls):
        T = ll.shape[0]
        assert (got[n, T:] == fill).all()
        if gs.status[n] != 0:
            assert lp[n] == 0.0 and (got[n] == fill).all()
            continue
        want_lp, want_n = want[n] if want and n in want else R.forward_backward(gs.graphs.export(n), ll)
        gamma = got[n, :T] - fill
        print("utt %d: T %d S %d logp %.6f want %.6f gamma err %.3g sum err %.3g" % (
            n, T, gs.graphs.num_states[n], lp[n], want_lp, np.abs(gamma - want_n).max(), np.abs(gamma.sum(1) - 1).max()))
        assert abs(lp[n] - want_lp) <= lp_rel * abs(want_lp) + 1e-4, (n, lp[n], want_lp)
        assert np.abs(gamma - want_n).max() <= 1e-4, (n, np.abs(gamma - want_n).max())
        assert np.abs(gamma.sum(1) - 1.0).max() <= 1e-4
    return lp, got


def test_parity_in_nan_buffer_and_adds_into_grad():
    aligner = _aligner()
    rng = np.random.default_rng(3)
    texts, frames = [[4], [2, 4], [3, 5, 4], [4, 4, 1, 3, 5]], [12, 47, 90, 150]
    gs = chain.graph_supervisions(aligner, texts, frames, transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0, 0, 0, 0], gs.errors
    lls = [(2.0 * rng.standard_normal((T, PDFS))).astype(np.float32) for T in frames]
    x = _poisoned(lls, PDFS)
    lp, got = _check_numerator(gs, lls, x)
    # the twin-of-den_forward_backward form returns the posteriors themselves; the call is bit-reproducible
    lp2, gamma = chain.num_graph_forward_backward(gs.graphs, x)
    lp3, gamma3 = chain.num_graph_forward_backward(gs.graphs, x)
    assert torch.equal(lp2, lp3) and torch.equal(gamma, gamma3) and np.array_equal(lp2.cpu().numpy(), lp)
    assert np.abs(gamma.cpu().numpy() - (got - 0.25)).max() <= 1e-6
    assert not gamma[:, max(frames):].any() and not gamma[0, frames[0]:].any()


def test_edges_minimum_length_one_frame_and_no_path():
    aligner = _aligner()
    rng = np.random.default_rng(4)
    words = [3, 4]
    Tmin = _min_frames(aligner, words)
    short = [5, 5, 5, 5]
    Tshort = _min_frames(aligner, short) - 1
    assert _min_frames(aligner, [6]) == 1
    texts, frames = [words, short, [6]], [Tmin, Tshort, 1]
    gs = chain.graph_supervisions(aligner, texts, frames, transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [chain.ALIGN_OK, chain.ALIGN_NO_PATH, chain.ALIGN_OK]
    lls = [(2.0 * rng.standard_normal((T, PDFS))).astype(np.float32) for T in frames]
    x = _poisoned(lls, PDFS)
    lp, got = _check_numerator(gs, lls, x)
    # at the minimum length the few paths left are enumerated: the log-probability is their sum, posteriors near 0 / 1
    g = gs.graphs.export(0)
    paths = R.enumerate_paths(g, Tmin)
    scores = np.asarray([sum(-float(g["weight"][k]) + float(lls[0][t, g["pdf"][k]]) for t, k in enumerate(p)) -
                         float(g["final"][g["dst"][p[-1]]]) for p in paths])
    want = scores.max() + np.log(np.exp(scores - scores.max()).sum())
    assert 1 <= len(paths) <= 4096 and abs(lp[0] - want) <= 1e-3 * abs(want) + 1e-4
    # the one-frame utterance: a single arc, posterior 1 on its pdf
    g1 = gs.graphs.export(2)
    assert np.abs((got[2, 0] - 0.25).sum() - 1.0) <= 1e-5 and set(np.flatnonzero(np.abs(got[2, 0] - 0.25) > 1e-6)) <= set(g1["pdf"].tolist())
    # the neighbours of the utterance without a path: bit-identical to the batch without it
    gs2 = chain.graph_supervisions(aligner, [texts[0], texts[2]], [frames[0], frames[2]], transition_scale=1.0, self_loop_scale=0.1)
    x2 = _poisoned([lls[0], lls[2]], PDFS)
    lp2, got2 = chain.num_graph_forward_backward(gs2, x2, grad=torch.full_like(x2, 0.25))
    lp2, got2 = lp2.cpu().numpy(), got2.cpu().numpy()
    for a, b in ((0, 0), (2, 1)):
        assert lp[a].tobytes() == lp2[b].tobytes()
        assert np.array_equal(got[a, :frames[a]].view(np.int32), got2[b, :frames[a]].view(np.int32))


@pytest.mark.parametrize("lds", ["1", "0"])
def test_more_states_than_lanes(monkeypatch, lds):
    monkeypatch.setenv("PK2_NUM_GRAPH_LDS", lds)
    aligner = _aligner()
    rng = np.random.default_rng(11)
    text = [int(w) for w in rng.integers(2, 6, size=26)]
    T = 420
    gs = chain.graph_supervisions(aligner, [text, [2, 4]], [T, 33], transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0, 0], gs.errors
    S = gs.graphs.num_states[0]
    assert S > 512 and S % 64 != 0, S
    assert bool(_lib.lib().pk2_num_graph_use_lds(gs.graphs._h)) == (lds == "1")
    lls = [(2.0 * rng.standard_normal((t, PDFS))).astype(np.float32) for t in (T, 33)]
    _check_numerator(gs, lls, _poisoned(lls, PDFS))


def test_long_and_peaked():
    """T = 1500 along a planted path (peak 8) with one 45.0 outlier: the per-frame scales and the double sums of their logs."""
    aligner = _aligner()
    rng = np.random.default_rng(9)
    text, T = [3, 5, 4, 2, 5], 1500
    gs = chain.graph_supervisions(aligner, [text], [T], transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0]
    g = gs.graphs.export(0)
    ll, _ = _planted(rng, g, T, PDFS)
    on_path = int(np.argmax(ll[700]))
    other = [int(p) for p in np.unique(g["pdf"]) if int(p) != on_path]
    ll[700, other[0]] = 45.0
    _check_numerator(gs, [ll], _poisoned([ll], PDFS))


def test_shared_pdfs_accumulate():
    """A monophone model over 6 pdfs: many states of a graph add into the same grad[t, p]."""
    aligner = _aligner(N=1, P=0, seed=5, num_pdfs=6)
    rng = np.random.default_rng(12)
    texts, frames = [[3, 5, 4], [5, 2, 5, 3, 4, 4]], [60, 131]
    gs = chain.graph_supervisions(aligner, texts, frames, transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0, 0]
    assert gs.graphs.num_states[1] > 10 * 6
    lls = [(2.0 * rng.standard_normal((T, 6))).astype(np.float32) for T in frames]
    _check_numerator(gs, lls, _poisoned(lls, 6))


@pytest.fixture(scope="module")
def objective_case():
    S, A = 200, 3000
    g = synth.den_graph_arcs(S, A, PDFS, 17)
    den = chain.DenominatorGraph(g, PDFS)
    ref = CR.DenGraphRef(g["num_states"], g["src"], g["dst"], g["pdf"], g["prob"], 0, PDFS)
    aligner = _aligner()
    rng = np.random.default_rng(21)
    texts = [[3, 5, 4], [5, 5, 5, 5], [2, 4], [4, 1, 3]]
    frames = [70, _min_frames(aligner, [5, 5, 5, 5]) - 1, 41, 96]
    gs = chain.graph_supervisions(aligner, texts, frames)       # default scales: only the lexicon's costs
    assert gs.status == [0, chain.ALIGN_NO_PATH, 0, 0]
    lls = [(2.0 * rng.standard_normal((T, PDFS))).astype(np.float32) for T in frames]
    leaky = 1e-4
    num, den_ = {}, {}
    for n, ll in enumerate(lls):
        if gs.status[n] == 0:
            num[n] = R.forward_backward(gs.graphs.export(n), ll)
            den_[n] = CR.den_forward_backward(ll.astype(np.float64), ref, leaky)[:2]
    return dict(den=den, ref=ref, aligner=aligner, gs=gs, texts=texts, frames=frames, lls=lls, leaky=leaky, num=num, den_ref=den_)


def _want(case, n, xent):
    (nlp, npost), (dlp, dpost) = case["num"][n], case["den_ref"][n]
    return nlp - dlp, nlp, dlp, (1.0 + xent) * npost - dpost


@pytest.mark.parametrize("xent", [0.0, 0.1])
def test_whole_objective(objective_case, xent):
    c = objective_case
    gs, frames, lls = c["gs"], c["frames"], c["lls"]
    x = _poisoned(lls, PDFS, fill=0.0)
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=c["leaky"], xent_regularize=xent)
    out, grad = chain.compute_chain_objf_and_deriv(opts, c["den"], gs, x)
    out_np, grad_np = out.cpu().numpy(), grad.cpu().numpy()
    total = 0.0
    for n, T in enumerate(frames):
        assert not grad_np[n, T:].any()
        if gs.status[n] != 0:       # no path: nothing from this utterance, the denominator included
            assert not out_np[:, n].any() and not grad_np[n].any()
            continue
        objf, nlp, dlp, want = _want(c, n, xent)
        total += objf
        print("utt %d: out %s want %s grad err %.3g" % (n, out_np[:, n], (objf, nlp, dlp), np.abs(grad_np[n, :T] - want).max()))
        assert abs(out_np[1, n] - nlp) <= 1e-3 * abs(nlp) + 1e-4
        assert abs(out_np[2, n] - dlp) <= 1e-3 * abs(dlp) + 1e-4
        assert abs(out_np[0, n] - objf) <= 1e-3 * abs(objf) + 1e-4
        assert np.abs(grad_np[n, :T] - want).max() <= 1e-4
    # operator form: the same three rows, their sum behind them, minus the derivative
    N = len(frames)
    out_op, neg = chain.compute_chain_objf_and_deriv(opts, c["den"], gs, x, operator_form=True)
    assert np.abs(out_op[:3 * N].cpu().numpy().reshape(3, N) - out_np).max() <= 1e-5 * abs(total)
    assert abs(float(out_op[3 * N]) - out_np[0].sum()) <= 1e-5 * abs(total) and abs(float(out_op[3 * N]) - total) <= 1e-3 * abs(total) + 1e-4
    assert np.abs(neg.cpu().numpy() + grad_np).max() <= 1e-6
    # the batch operator and the per-utterance operator hand the same (negated) gradient to autograd
    xb = x.detach().clone().requires_grad_(True)
    loss = ops.ChainObjtiveBatch.apply(xb, c["den"], gs, opts)
    loss.backward()
    assert abs(float(loss.detach()) - float(out_op[3 * N])) <= 1e-5 * abs(total) and np.abs(xb.grad.cpu().numpy() + grad_np).max() <= 1e-6
    n = 2
    one = chain.graph_supervisions(c["aligner"], [c["texts"][n]], [frames[n]])
    xl = torch.from_numpy(lls[n]).cuda().requires_grad_(True)
    obj = ops.ChainObjtiveFunction.apply(xl, c["den"], one, opts)
    obj.backward()
    objf, _, _, want = _want(c, n, xent)
    assert abs(float(obj.detach()) - objf) <= 1e-3 * abs(objf) + 1e-4
    assert np.abs(xl.grad.cpu().numpy() + want).max() <= 1e-4


def test_bad_arguments_fail_loudly():
    aligner = _aligner()
    gs = chain.graph_supervisions(aligner, [[3, 4]], [40])
    L = _lib.lib()
    x = torch.zeros(1, 40, PDFS, device="cuda")
    dev = gs.graphs.to_device(x.device)
    need = L.pk2_num_graph_workspace_bytes(gs.graphs._h)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    lp = torch.empty(1, device="cuda")
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    args = lambda P, wsb, g=x: (gs.graphs._h, _lib.ptr(dev), _lib.ptr(x), x.stride(0), x.stride(1), P, 40, 1.0, _lib.ptr(g),   # noqa: E731
                                x.stride(0), x.stride(1), _lib.ptr(lp), _lib.ptr(st), _lib.ptr(ws), wsb, None)
    max_pdf = int(gs.graphs.export(0)["pdf"].max())
    with pytest.raises(_lib.Pk2Error, match="columns"):
        _lib.check(L.pk2_num_graph_fwd_bwd(*args(max_pdf, need)))
    with pytest.raises(_lib.Pk2Error, match="workspace"):
        _lib.check(L.pk2_num_graph_fwd_bwd(*args(PDFS, need - 256)))
    with pytest.raises(_lib.Pk2Error, match="null"):
        _lib.check(L.pk2_num_graph_fwd_bwd(*args(PDFS, need, g=None)))
    small = chain.DenominatorGraph(synth.den_graph_arcs(20, 100, max_pdf, 1), max_pdf)
    with pytest.raises(_lib.Pk2Error, match="pdfs"):
        chain.compute_chain_objf_and_deriv(chain.ChainTrainingOptions(), small, gs, x[:, :, :max_pdf].contiguous())


# ---------------------------------------------------------------- graphs beyond 1024 states (tests/graph_cases.py)
def _supervisions(texts, frames):
    gs = chain.graph_supervisions(GC.numerator_aligner(), texts, frames, transition_scale=1.0, self_loop_scale=0.1)
    return gs


def _use_lds(gs):
    return bool(_lib.lib().pk2_num_graph_use_lds(gs.graphs._h))


def _twice_equal(gs, x):
    """The call claims bit-reproducibility: two calls, both outputs equal."""
    a, b = chain.num_graph_forward_backward(gs, x), chain.num_graph_forward_backward(gs, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ladder_numerator(monkeypatch, k):
    """Rung 1: a third and a fourth state per lane (past the two whose factors are prefetched) in both chains, ng_chains
    above 64 KiB of LDS, and the same graph forced into global memory.  Rung 2: ng_chains within 16 KiB of the LDS limit.
    Rung 3: global memory chosen by size."""
    monkeypatch.delenv("PK2_NUM_GRAPH_LDS", raising=False)
    words, T, x_np, want = GC.numerator_case(k)
    gs = _supervisions([words], [T])
    assert gs.status == [0], gs.errors
    S, A = gs.graphs.num_states[0], gs.graphs.num_arcs[0]
    GC.assert_rung(k, S)
    lds = GC.chains_lds(S, A)
    if k == 1:
        assert S > 3 * GC.THREADS and GC.LDS_OPT_IN < lds <= GC.LDS_LIMIT and _use_lds(gs)
    elif k == 2:
        assert GC.LDS_LIMIT - 16 * 1024 < lds <= GC.LDS_LIMIT and _use_lds(gs)
    else:
        assert lds > GC.LDS_LIMIT and not _use_lds(gs)
    print("rung %d: S %d A %d T %d, ng_chains LDS %d -> %s, ng_post LDS %d" % (
        k, S, A, T, lds, "LDS" if _use_lds(gs) else "global", GC.post_lds(S)))
    x = _poisoned([x_np], PDFS)
    _check_numerator(gs, [x_np], x, want={0: want})
    _twice_equal(gs, x)
    if k == 1:
        in_lds = chain.num_graph_forward_backward(gs, x)
        monkeypatch.setenv("PK2_NUM_GRAPH_LDS", "0")
        assert not _use_lds(gs)
        _check_numerator(gs, [x_np], x, want={0: want})
        _twice_equal(gs, x)
        # the two routes are one arithmetic: an utterance must not change with the size of its neighbours
        in_global = chain.num_graph_forward_backward(gs, x)
        assert torch.equal(in_lds[0], in_global[0]) and torch.equal(in_lds[1], in_global[1])


def test_widest_numerator_in_a_mixed_batch(monkeypatch):
    """Rung 4: ng_post above 64 KiB of LDS, the chains in global memory, next to a two-word utterance and one without a
    path; the neighbours are bit-identical to the batch without the large graph."""
    monkeypatch.delenv("PK2_NUM_GRAPH_LDS", raising=False)
    words, T, x_np, want = GC.numerator_case(4)
    aligner = GC.numerator_aligner()
    short = [5, 5, 5, 5]
    texts, frames = [words, [2, 4], short], [T, 33, _min_frames(aligner, short) - 1]
    gs = _supervisions(texts, frames)
    assert gs.status == [0, 0, chain.ALIGN_NO_PATH], gs.errors
    S, A = gs.graphs.num_states[0], gs.graphs.num_arcs[0]
    GC.assert_rung(4, S)
    assert 8 * S > GC.LDS_OPT_IN and GC.post_lds(max(gs.graphs.num_states)) > GC.LDS_OPT_IN
    assert GC.chains_lds(S, A) > GC.LDS_LIMIT and not _use_lds(gs)
    print("rung 4: S %d A %d T %d, ng_chains LDS %d -> global, ng_post LDS %d" % (S, A, T, GC.chains_lds(S, A), GC.post_lds(S)))
    rng = np.random.default_rng(41)
    lls = [x_np] + [(2.0 * rng.standard_normal((t, PDFS))).astype(np.float32) for t in frames[1:]]
    x = _poisoned(lls, PDFS)
    lp, got = _check_numerator(gs, lls, x, want={0: want})
    _twice_equal(gs, x)
    gs2 = _supervisions(texts[1:], frames[1:])
    assert _use_lds(gs2)
    x2 = _poisoned(lls[1:], PDFS)
    lp2, got2 = chain.num_graph_forward_backward(gs2, x2, grad=torch.full_like(x2, 0.25))
    lp2, got2 = lp2.cpu().numpy(), got2.cpu().numpy()
    for n in (1, 2):
        assert lp[n].tobytes() == lp2[n - 1].tobytes()
        assert np.array_equal(got[n, :frames[n]].view(np.int32), got2[n - 1, :frames[n]].view(np.int32))


def test_whole_objective_large_graph(objective_case):
    """The rung-1 graph inside the fused entry (its workspace is carved differently from the stand-alone one), on the
    200-state denominator; the tolerances of test_whole_objective."""
    c = objective_case
    words, T, x_np, (nlp, npost) = GC.numerator_case(1)
    gs = _supervisions([words], [T])
    assert gs.status == [0]
    GC.assert_rung(1, gs.graphs.num_states[0])
    dlp, dpost = CR.den_forward_backward(x_np.astype(np.float64), c["ref"], c["leaky"])[:2]
    xent = 0.1
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=c["leaky"], xent_regularize=xent)
    out, grad = chain.compute_chain_objf_and_deriv(opts, c["den"], gs, _poisoned([x_np], PDFS, fill=0.0))
    out_np, grad_np = out.cpu().numpy(), grad.cpu().numpy()
    objf, want = nlp - dlp, (1.0 + xent) * npost - dpost
    print("out %s want %s grad err %.3g" % (out_np[:, 0], (objf, nlp, dlp), np.abs(grad_np[0, :T] - want).max()))
    assert abs(out_np[1, 0] - nlp) <= 1e-3 * abs(nlp) + 1e-4
    assert abs(out_np[2, 0] - dlp) <= 1e-3 * abs(dlp) + 1e-4
    assert abs(out_np[0, 0] - objf) <= 1e-3 * abs(objf) + 1e-4
    assert np.abs(grad_np[0, :T] - want).max() <= 1e-4
    assert not grad_np[0, T:].any()


# ---------------------------------------------------------------- the range of the per-frame scale
def test_scale_range_gap_60():
    """A pdf of an unreachable state 60 above every other logit of its frame -- the widest spread the denominator's +-30
    clamp lets through -- at frame 0 and at a middle frame: every live factor of those frames is e^-60 or less, the
    frame's alpha sum with it, and the posterior pass multiplies across that.  The normal tolerances hold."""
    c = GC.scale_range_case(60.0)
    gs = _supervisions([c["words"]], [c["T"]])
    assert gs.status == [0]
    _check_numerator(gs, [c["x"]], _poisoned([c["x"]], PDFS), want={0: c["want"]})


def _meets_tolerances_or_is_abandoned(oc, texts, frames, lls, want):
    """The last utterance of the batch is one the float32 range of the numerator may not hold.  Through the objective it
    either meets the tolerances or is abandoned cleanly -- objective -10 T weight, gradient rows exactly zero, nothing
    non-finite in the gradient, never a finite log-probability that is wrong -- and the utterances before it are
    bit-identical to the batch without it.  Returns "met" or "abandoned"."""
    n, T = len(texts) - 1, frames[-1]
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=oc["leaky"], xent_regularize=0.0)
    gs = _supervisions(texts, frames)
    assert gs.status == [0] * (n + 1)
    out, grad = chain.compute_chain_objf_and_deriv(opts, oc["den"], gs, _poisoned(lls, PDFS, fill=0.0))
    out, grad = out.cpu().numpy(), grad.cpu().numpy()
    gs2 = _supervisions(texts[:n], frames[:n])
    out2, grad2 = chain.compute_chain_objf_and_deriv(opts, oc["den"], gs2, _poisoned(lls[:n], PDFS, fill=0.0))
    out2, grad2 = out2.cpu().numpy(), grad2.cpu().numpy()
    want_lp, want_post = want
    print("last utterance: out %s (oracle log p_num %.6f), |grad| max %s" % (out[:, n], want_lp, np.abs(grad[n]).max()))
    assert np.isfinite(grad).all()
    if np.isfinite(out[1, n]):          # a finite numerator log-probability is a right one
        assert abs(out[1, n] - want_lp) <= 1e-3 * abs(want_lp) + 1e-4, (out[1, n], want_lp)
    if out[0, n] == np.float32(-10.0 * T * gs.weight) and not grad[n].any():
        outcome = "abandoned"
    else:
        dlp, dpost = CR.den_forward_backward(lls[n].astype(np.float64), oc["ref"], oc["leaky"])[:2]
        assert abs(out[1, n] - want_lp) <= 1e-3 * abs(want_lp) + 1e-4
        assert abs(out[2, n] - dlp) <= 1e-3 * abs(dlp) + 1e-4
        assert abs(out[0, n] - (want_lp - dlp)) <= 1e-3 * abs(want_lp - dlp) + 1e-4
        assert np.abs(grad[n, :T] - (want_post - dpost)).max() <= 1e-4
        outcome = "met"
    for m in range(n):
        assert np.array_equal(out[:, m].view(np.int32), out2[:, m].view(np.int32)), (m, out[:, m], out2[:, m])
        assert np.array_equal(grad[m, :frames[m]].view(np.int32), grad2[m, :frames[m]].view(np.int32)), m
        assert not grad[m, frames[m]:].any()
    print("outcome:", outcome)
    return outcome


def test_scale_range_gap_200(objective_case):
    """The same with a gap of 200, beyond what expf can represent: see _meets_tolerances_or_is_abandoned."""
    c, oc = GC.scale_range_case(200.0), objective_case
    texts, frames = [oc["texts"][0], oc["texts"][2], c["words"]], [oc["frames"][0], oc["frames"][2], c["T"]]
    _meets_tolerances_or_is_abandoned(oc, texts, frames, [oc["lls"][0], oc["lls"][2], c["x"]], c["want"])


def test_near_minimum_length_on_noise(objective_case):
    """Rung 1 at 50 frames above its minimum length on noise alone (graph_cases.noise_only_case): the paths that finish
    hold e^-479 of the forward mass, far below what float32 probability space can carry next to the rest.  The
    numerator cannot be right there; it must not be wrong quietly."""
    oc = objective_case
    words, T, x_np, want = GC.noise_only_case()
    texts, frames = [oc["texts"][2], words], [oc["frames"][2], T]
    _meets_tolerances_or_is_abandoned(oc, texts, frames, [oc["lls"][2], x_np], want)
