"""The supervised LF-MMI numerator (csrc/chain_num.h) on every carrier the host code can pick for it, against the float64
oracle on the supervisions of tests/num_cases.py, at bounds measured on the CPU (num_cases.POST_BOUND / LP_BOUND: 4 x the error
of a float32 restatement of the same recursion).  Every test asserts the route it was written for (chain.last_num_route()).

Carriers:  A stand-alone staged, B stand-alone unstaged (256 threads), C / D inside the occupancy launch
(two waves staged / one wave unstaged; LDS-row and gather variant of that kernel), E tasks of the persistent launch (two waves).

The numerator's posteriors are isolated from the combined gradient with the denominator occupancies of
chain.den_forward_backward under the same environment, post = (grad + w gamma + w l2 x) / (w (1 + xent)), after asserting that
two denominator calls are bit-equal on that route.  On the general family (float atomics) they are not: there the whole
gradient is compared with the oracle at the 1e-4 of test_gpu_chain.py, and the log-probability stays tight.

Graphs: those of test_gpu_chain.py::test_denominator_matches_oracle.  The persistent table of _mk(200, 3000, 40) has 256
floats (1 KB) and `narrow` staged needs 2.7 KB, so nothing rides there: route E runs on the smallest of that test's graphs on
which `narrow` rides, _mk(2000, 60000, 600, seed=2000) (table: 8 KB), with the cases' 40 pdfs as the first 40 of its 600.
`edges` (64 KB staged), `long_staged`, and the unstaged cases ride on no graph of that test: E gets the thresholds of the
two-wave routine (16 | 17 and 64 | 65 arcs in a frame: it has no others) from `edges_small`."""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import num_cases as nc
from oracle import chain_ref as R
from pykaldi2_amd import _lib, chain
# (one copy of the graph builder: the module imports without a GPU)
from test_gpu_chain import _mk

pytestmark = pytest.mark.gpu

LEAKY = 1e-4
SWITCHES = ("PK2_NUM_SIDE", "PK2_SIDE_STREAM", "PK2_DEN_MODE", "PK2_DEN_NUM_RIDE", "PK2_DEN_GAMMA_GATHER", "PK2_DEN_PERSIST")


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """small: P = 40 (state-x by itself, general when forced); ride: the graph whose persistent table takes `narrow`."""
    return _mk(200, 3000, 40, seed=200) if kind == "small" else _mk(2000, 60000, 600, seed=2000)


class Batch:
    """Cases side by side in one ragged minibatch (never modified once made): logits [N, Tmax, P] whose first 40 columns hold
    each case's own logits on its frames and noise elsewhere -- past the lengths too: nothing may read those."""

    def __init__(self, specs, P):
        self.cases = [nc.case(n, s) for n, s in specs]
        self.specs, self.P, self.N = list(specs), P, len(specs)
        self.lens = [c.T for c in self.cases]
        rng = np.random.default_rng(len(specs) * 1000 + P)
        self.x = rng.normal(0.0, 3.0, size=(self.N, max(self.lens), P)).astype(np.float32)
        for n, c in enumerate(self.cases):
            self.x[n, :c.T, :nc.P] = c.logits
        self.staged = nc.is_staged(self.cases)
        self.lds = nc.staged_lds_bytes(self.cases) if self.staged else 4 * (2 * max(c.fst["num_states"] for c in self.cases) + 8)

    def sups(self, weight=1.0):
        return [chain.Supervision(c.fst, weight=weight, label_dim=self.P) for c in self.cases]

    def want(self, n):
        """-> (log p_num, posteriors [T, P]) of the oracle for sequence n."""
        lp, post = nc.oracle(*self.specs[n])
        full = np.zeros((self.lens[n], self.P))
        full[:, :nc.P] = post
        return lp, full

    def no_arc(self, n):
        """[T, P] mask of the pdfs that no arc of the frame carries."""
        c = self.cases[n]
        m = np.ones((c.T, self.P), bool)
        m[np.repeat(np.arange(c.T), c.frame_arcs), c.fst["pdf"]] = False
        return m


@functools.lru_cache(maxsize=None)
def _batch(which, P=nc.P):
    specs = {
        # N = 9, ragged: three groups of 4 with padding sequences, a second InfoPack; staged
        "1": [("edges", 0), ("narrow", 0), ("one_frame", 0), ("peaked", 0), ("dead_ends", 0), ("narrow", 1), ("edges", 1),
              ("one_frame", 1), ("dead_ends", 1)],
        # the largest sequence has 7961 arcs: unstaged
        "2": [("unstaged", 0), ("narrow", 0), ("one_frame", 0)],
        # what fits the 8 KB table of the `ride` graph, N = 9 again
        "E": [("edges_small", 0), ("narrow", 0), ("one_frame", 0), ("dead_ends", 0), ("edges_small", 1), ("narrow", 1),
              ("dead_ends", 1), ("one_frame", 1), ("narrow", 2)],
        "long": [("long", 0)], "long_staged": [("long_staged", 0)], "max_states": [("max_states", 0)],
        "too_many_states": [("too_many_states", 0)],
        "narrow21": [("narrow", s) for s in range(21)], "narrow22": [("narrow", s) for s in range(22)],
        "narrow2": [("narrow", 0), ("narrow", 1)],
    }[which]
    return Batch(specs, P)


def _den_twice(G, x, lens):
    """The denominator alone, twice: the occupancies the posteriors are isolated with must be reproducible to the bit."""
    lp1, g1 = chain.den_forward_backward(G, x, lens, LEAKY)
    lp2, g2 = chain.den_forward_backward(G, x, lens, LEAKY)
    same = torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(lp1.view(torch.int32), lp2.view(torch.int32))
    assert same, "denominator occupancies differ between two calls on this route"
    return g1.cpu().numpy().astype(np.float64)


def _run(b, G, opts=None, weight=1.0, x=None, operator_form=False):
    x = torch.from_numpy(b.x).cuda() if x is None else x
    opts = opts or chain.ChainTrainingOptions(leaky_hmm_coefficient=LEAKY)
    out, grad = chain.compute_chain_objf_and_deriv(opts, G, b.sups(weight), x, operator_form=operator_form)
    route = chain.last_num_route()
    torch.cuda.synchronize()
    return out.cpu().numpy(), grad.cpu().numpy(), route, x


def _assert_route(route, b, carrier, threads):
    want = dict(staged=b.staged, carrier=carrier, threads=threads, lds_bytes=b.lds)
    assert route == want, (route, want)


def _check_lp(b, out):
    for n in range(b.N):
        lp = b.want(n)[0]
        err = abs(float(out[1, n]) - lp) / max(1.0, abs(lp))
        print("seq %d %-12s lp %.6f error %.3g (bound %.3g)" % (n, b.specs[n][0], lp, err, nc.LP_BOUND))
        assert err <= nc.LP_BOUND, (n, b.specs[n], out[1, n], lp)


def _check_tight(b, G, out, grad, x, w=1.0, xent=0.0, l2=0.0):
    """log p_num, the isolated posteriors, their row sums, the pdfs on no arc (exact when l2 = 0) and the padding frames."""
    _check_lp(b, out)
    gamma = _den_twice(G, x, b.lens)
    g64 = grad.astype(np.float64)
    for n, T in enumerate(b.lens):
        post = (g64[n, :T] + w * gamma[n, :T] + w * l2 * b.x[n, :T].astype(np.float64)) / (w * (1.0 + xent))
        want = b.want(n)[1]
        err, rows = np.abs(post - want).max(), np.abs(post.sum(1) - 1.0).max()
        print("seq %d %-12s posteriors: error %.3g, row sums %.3g (bound %.3g)" % (n, b.specs[n][0], err, rows, nc.POST_BOUND))
        assert err <= nc.POST_BOUND and rows <= nc.POST_BOUND, (n, b.specs[n], err, rows)
        if l2 == 0.0:
            m = b.no_arc(n)
            assert (grad[n, :T][m] == (-np.float32(w) * gamma[n, :T].astype(np.float32))[m]).all(), n
        assert not grad[n, T:].any(), n


def _check_whole(b, ref, out, grad, w=1.0, xent=0.0, l2=0.0, bad=()):
    """Objective and the whole gradient against the oracle at the bounds of test_gpu_chain.py (1e-3 relative, 1e-4 absolute)."""
    for n, T in enumerate(b.lens):
        x = b.x[n, :T].astype(np.float64)
        objf, want, aux = R.chain_objf_and_deriv(x, ref, b.cases[n].ref, leaky=LEAKY, xent_regularize=xent, weight=w,
                                                 l2_regularize=l2)
        assert aux["ok"] == (n not in bad), (n, aux)
        if n in bad:        # abandoned: -10 per frame, and a derivative that is the l2 term alone
            assert out[0, n] == np.float32(-10.0 * w * T)
            np.testing.assert_allclose(grad[n, :T], want, rtol=0, atol=1e-9, equal_nan=True)
            assert l2 != 0.0 or not grad[n, :T].any()
        else:
            assert abs(out[0, n] - objf) <= 1e-3 * abs(objf), (n, out[0, n], objf)
            assert abs(out[2, n] - aux["den"]) <= 1e-3 * abs(aux["den"])
            err = np.abs(grad[n, :T] - want).max()
            assert err < 1e-4, (n, err)
        assert not grad[n, T:].any(), n


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------------------------------------------------
# routes A - D on the 40-pdf graph
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = {
    # name: (environment, carrier, threads of the staged batch, threads of the unstaged one)
    "side": (dict(PK2_NUM_SIDE="1"), "side_stream", 256, 256),
    "side_stream": (dict(PK2_SIDE_STREAM="1"), "side_stream", 256, 256),
    "general": (dict(PK2_DEN_MODE="general"), "stand_alone", 256, 256),
    "noride": (dict(PK2_DEN_NUM_RIDE="0"), "occupancy_lds_row", 128, 64),
    "noride_gather": (dict(PK2_DEN_NUM_RIDE="0", PK2_DEN_GAMMA_GATHER="1"), "occupancy_gather", 128, 64),
    "frames": (dict(PK2_DEN_PERSIST="0"), "occupancy_lds_row", 128, 64),
    # the staged need of either batch is beyond the 1 KB table of this graph: the persistent launch declines
    "default_too_big_to_ride": (dict(), "occupancy_lds_row", 128, 64),
}


@pytest.mark.parametrize("which", ["1", "2"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_routes_on_the_small_graph(route, which, monkeypatch):
    _clear(monkeypatch)
    env, carrier, t_staged, t_unstaged = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, G, ref = _graph("small")
    b = _batch(which)
    assert b.staged == (which == "1")
    pl = G.plan(b.N, max(b.lens))
    assert pl["family"] == (0 if route == "general" else 1) and pl["form"] == (0 if route in ("general", "frames") else 2), pl
    if route == "frames":
        assert pl["NG"] == 4
    out, grad, r, x = _run(b, G)
    _assert_route(r, b, carrier, t_staged if b.staged else t_unstaged)
    if route == "general":
        _check_lp(b, out)
        _check_whole(b, ref, out, grad)
    else:
        _check_tight(b, G, out, grad, x)


@pytest.mark.parametrize("which,route,threads", [
    ("long", "side", 256), ("long", "noride", 64), ("long_staged", "side", 256), ("long_staged", "noride", 128),
    ("long_staged", "noride_gather", 128), ("max_states", "side", 256), ("max_states", "noride", 64),
    ("max_states", "noride_gather", 64)])
def test_long_and_largest_sequences_alone(which, route, threads, monkeypatch):
    """602 frames (scale drift) and kNumMaxStates states (frames of 8999 arcs: the recompute branch of both one-routine
    bodies), N = 1.  None of them can ride in the persistent launch (their LDS need is beyond the table of every graph of
    test_denominator_matches_oracle): routes A - D."""
    _clear(monkeypatch)
    env, carrier, _, _ = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, G, ref = _graph("small")
    b = _batch(which)
    assert b.staged == (which == "long_staged")
    out, grad, r, x = _run(b, G)
    _assert_route(r, b, carrier, threads)
    _check_tight(b, G, out, grad, x)


def test_too_many_states_is_refused_and_the_next_call_is_correct(monkeypatch):
    _clear(monkeypatch)
    g, G, ref = _graph("small")
    b = _batch("too_many_states")
    with pytest.raises(_lib.Pk2Error, match="18001 states"):
        _run(b, G)
    assert chain.last_num_route()["carrier"] == "none"
    b = _batch("2")
    out, grad, r, x = _run(b, G)
    _assert_route(r, b, "occupancy_lds_row", 64)
    _check_tight(b, G, out, grad, x)


# ---------------------------------------------------------------------------------------------------------------------
# route E
# ---------------------------------------------------------------------------------------------------------------------
def _warm_up(G, P):
    """The first persistent launch of a process is verified and carries no numerator: one call in front.  In a process where
    an earlier test has had that launch, this one rides already (test_first_persistent_launch_... pins the rule itself)."""
    b = _batch("narrow2", P)
    out, grad, r, x = _run(b, G)
    assert r["carrier"] in ("occupancy_lds_row", "persistent") and r["staged"], r


def test_persistent_launch_carries_the_numerator(monkeypatch):
    _clear(monkeypatch)
    g, G, ref = _graph("ride")
    P = G.num_pdfs()
    _warm_up(G, P)
    b = _batch("E", P)
    lay = [G.debug_persist2(w)["tfloats"] for w in (0, 1)]
    assert G.plan(b.N, max(b.lens))["form"] == 2 and b.staged and b.lds <= 4 * max(lay), (b.lds, lay)
    out, grad, r, x = _run(b, G)
    _assert_route(r, b, "persistent", 128)
    _check_tight(b, G, out, grad, x)
    # the same graph with the ride switched off: the occupancy launch takes it
    monkeypatch.setenv("PK2_DEN_NUM_RIDE", "0")
    out2, grad2, r2, _ = _run(b, G)
    _assert_route(r2, b, "occupancy_lds_row", 128)
    _check_tight(b, G, out2, grad2, x)


@pytest.mark.parametrize("N,rides", [(21, True), (22, False)])
def test_persistent_launch_task_limit(N, rides, monkeypatch):
    """2 N recursions and N numerators share the 64 tasks of a launch (den_persist_tasks / den_persist2_launch): 21 sequences
    ride, 22 do not -- the plan stays on the second form up to 32."""
    _clear(monkeypatch)
    g, G, ref = _graph("ride")
    P = G.num_pdfs()
    _warm_up(G, P)
    b = _batch("narrow%d" % N, P)
    assert G.plan(N, max(b.lens))["form"] == 2
    out, grad, r, x = _run(b, G)
    _assert_route(r, b, "persistent" if rides else "occupancy_lds_row", 128)
    _check_tight(b, G, out, grad, x)


_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import num_cases as nc
import test_gpu_chain_num as t
from pykaldi2_amd import chain
g, G, ref = t._graph("ride")
b = t._batch("narrow2", G.num_pdfs())
out, grad, r, x = t._run(b, G)
t._assert_route(r, b, "occupancy_lds_row", 128)       # the first, verified launch of the process: no numerator inside
t._check_lp(b, out)
out, grad, r, x = t._run(b, G)
t._assert_route(r, b, "persistent", 128)
t._check_tight(b, G, out, grad, x)
print("child ok")
"""


def test_first_persistent_launch_of_a_process_carries_no_numerator():
    """In a process of its own (the rule is per process): the first call takes the occupancy launch, the second one rides."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    p = subprocess.run([sys.executable, "-c", _CHILD % (root, os.path.join(root, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------
# objective options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,xent,l2", [(0.5, 0.1, 5e-4), (0.5, 0.0, 0.0), (1.0, 0.1, 0.0), (1.0, 0.0, 5e-4)])
@pytest.mark.parametrize("operator_form", [False, True])
def test_objective_options(w, xent, l2, operator_form, monkeypatch):
    """Supervision.weight, xent_regularize and l2_regularize together and one at a time, against R.chain_objf_and_deriv and
    (posteriors in isolation) at the tight bound; sequence 1 is abandoned through a NaN logit: by SURVEY A.1 its derivative
    is zeroed (step 4) BEFORE the l2 term is subtracted (step 5).  operator_form: minus the derivative, and out[3N] = the sum
    of the objectives in the kernel's fixed order."""
    _clear(monkeypatch)
    g, G, ref = _graph("small")
    base = _batch("1")
    b = Batch(base.specs[:5], nc.P)
    xb = b.x.copy()
    c = b.cases[1]
    xb[1, 3, c.fst["pdf"][c.fst["frame_offsets"][3]]] = np.nan
    x = torch.from_numpy(xb).cuda()
    opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=LEAKY, xent_regularize=xent, l2_regularize=l2)
    out, grad, r, _ = _run(b, G, opts, w, x, operator_form)
    _assert_route(r, b, "occupancy_lds_row", 128)
    N = b.N
    if operator_form:
        total, out, grad = out[3 * N], out[:3 * N].reshape(3, N), -grad
        v = np.zeros(64, np.float32)
        v[:N] = out[0]
        for o in (32, 16, 8, 4, 2, 1):          # wave_sum: the xor butterfly of the first wave (the other three hold zeros)
            v = v + v[np.arange(64) ^ o]
        assert total == v[0], (total, v[0])
        exact = out[0].astype(np.float64).sum()
        assert abs(float(total) - exact) <= N * np.spacing(np.float32(abs(exact)))
    bx = copy.copy(b)           # (the same batch with the logits that were run)
    bx.x = xb
    _check_whole(bx, ref, out, grad, w, xent, l2, bad=(1,))
    # the healthy sequences once more, tightly (the abandoned one has no posteriors)
    gamma = _den_twice(G, x, b.lens)
    for n, T in enumerate(b.lens):
        if n == 1:
            continue
        post = (grad[n, :T].astype(np.float64) + w * gamma[n, :T] + w * l2 * xb[n, :T].astype(np.float64)) / (w * (1.0 + xent))
        err = np.abs(post - b.want(n)[1]).max()
        print("seq %d posteriors: error %.3g (bound %.3g)" % (n, err, nc.POST_BOUND))
        assert err <= nc.POST_BOUND, (n, err)
        lp = b.want(n)[0]
        assert abs(float(out[1, n]) - lp) <= nc.LP_BOUND * max(1.0, abs(lp))


# ---------------------------------------------------------------------------------------------------------------------
# strides and poisoning, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["side", "noride", "persistent"])
def test_strided_buffers_and_poisoned_padding(route, monkeypatch):
    """Batch-major logits with row padding, a time-major NaN-filled gradient buffer whose frame stride exceeds N * P and that
    has rows for more sequences than the batch: the results are those of the contiguous call -- to the bit where the denominator
    alone writes (log p_den, the pdfs on no arc), inside the numerator's bounds where its float atomics add in a free order --,
    padding columns and the rows of sequences past N keep their NaN bit pattern."""
    _clear(monkeypatch)
    g, G, ref = _graph("ride" if route == "persistent" else "small")
    P = G.num_pdfs()
    if route == "persistent":
        _warm_up(G, P)
        carrier, threads, b = "persistent", 128, _batch("E", P)
    else:
        env, carrier, threads, _ = ROUTES[route]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        b = _batch("1", P)
    out0, grad0, r0, x0 = _run(b, G)
    _assert_route(r0, b, carrier, threads)
    N, Tm = b.N, max(b.lens)
    pad_l, pad_g, extra = 24, 8, 2
    xl = torch.full((N, Tm, P + pad_l), float("nan"), device="cuda")
    xl[:, :, :P] = x0
    x = xl[:, :, :P]                                   # [N, Tm, P], frame stride P + 24
    poison = np.uint32(0x7fc00abc)
    gbuf = torch.from_numpy(np.full((Tm, N + extra, P + pad_g), poison, np.uint32).view(np.float32)).cuda()
    gv = gbuf[:, :N, :P].transpose(0, 1)               # [N, Tm, P], time-major underneath
    sb = chain._SupervisionBatch(b.sups(), x.device)
    L = _lib.lib()
    ws = chain._workspace(x.device, L.pk2_chain_workspace_bytes(G._h, N, Tm, max(sb.total_arcs, int(sb.lengths.sum()) + N)))
    out = torch.empty(3, N, dtype=torch.float32, device="cuda")
    _lib.check(L.pk2_chain_objf_and_deriv(G._h, _lib.ptr(x), x.stride(0), x.stride(1), _lib.ptr(sb.lengths), N, C.byref(sb.struct),
                                          LEAKY, 0.0, 0.0, 1.0, _lib.ptr(gv), gv.stride(0), gv.stride(1), _lib.ptr(out),
                                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    r = chain.last_num_route()
    torch.cuda.synchronize()
    _assert_route(r, b, carrier, threads)
    out, full = out.cpu().numpy(), gbuf.cpu().numpy()
    grad = full[:, :N, :P].transpose(1, 0, 2)
    # (log p_den to the bit; log p_num sums float atomics whose order is free: inside its bound)
    assert (out[2] == out0[2]).all() and (np.abs(out[1] - out0[1]) <= nc.LP_BOUND * np.maximum(1.0, np.abs(out0[1]))).all()
    for n, T in enumerate(b.lens):
        m = b.no_arc(n)
        assert (grad[n, :T][m] == grad0[n, :T][m]).all() and np.abs(grad[n, :T] - grad0[n, :T]).max() <= nc.POST_BOUND, n
        assert not grad[n, T:Tm].any(), n
    bits = full.view(np.uint32)
    assert (bits[:, :, P:] == poison).all() and (bits[:, N:, :] == poison).all()
    _check_tight(b, G, out, grad, x0)
