"""Transcript graphs beyond 1024 states for the device Viterbi (csrc/align_viterbi.hip, tests/test_gpu_align.py) and the
alignment-free numerator (csrc/chain_num_graph.hip, tests/test_gpu_num_graph.py): a ladder of transcripts whose graphs land
on every code path the two kernels choose from the largest graph of a batch, the formulas of those choices restated so
that a test asserts its route from the graph itself, and the CPU references, computed once per process and shared.
Test infrastructure only; everything here runs on the CPU (tests/test_graph_cases.py checks the host-only parts)."""
import functools

import numpy as np

from pykaldi2_amd import chain

import num_graph_ref as R
from test_align_graph import PRONS, emulate_viterbi, kaldi_like_lexicon, make_model

PDFS = 60
ASCALE = 0.1
THREADS = 512                       # align_internal.h: kAlignThreads, the lanes the states are spread over
MAX_STATES = 32 * THREADS           # kAlignMaxStates
LDS_LIMIT = 160 * 1024 - 1024       # kLdsLimit of both kernels: dynamic LDS a workgroup may ask for
LDS_OPT_IN = 64 * 1024              # above this a launch needs hipFuncAttributeMaxDynamicSharedMemorySize
PRONS1 = PRONS + [(6, [7], 0.2, None)]      # phone 7 has the one-state chain topology: a word of one frame

# rung -> (words of the transcript, the open-closed range its state count must fall in): states per thread 4, 8, 16, 32
RUNGS = {1: (100, 1024, 2048), 2: (200, 2048, 4096), 3: (300, 4096, 8192), 4: (400, 8192, MAX_STATES)}
# Beams that bind on the ladder's log-likelihoods (rung_loglikes): below the margin of the unpruned best path, so that
# path is pruned, and wide enough that another one reaches a final state.  Found on the CPU with emulate_viterbi's trace;
# viterbi_reference asserts both properties again.
BINDING_BEAM = {1: 68.15, 2: 124.7, 3: 206.9, 4: 239.95}


def up16(n):
    return (n + 15) // 16 * 16


def viterbi_lds(S, A):
    """align_viterbi.hip: two cost vectors, in-arc offsets, arcx and weights."""
    return up16(12 * S + 4 + 8 * A)


def chains_lds(S, A):
    """chain_num_graph.hip, ng_chains: the beta chain's need (two vectors of 2 S, out-arc offsets, arcs, e^-w)."""
    return up16(20 * S + 4 + 8 * A)


def post_lds(S):
    """chain_num_graph.hip, ng_post: q of both arc kinds per state."""
    return up16(8 * S)


def states_per_thread(S):
    spt = 1
    while spt * THREADS < S:
        spt *= 2
    return spt


def ladder_words(n):
    return [int(w) for w in np.random.default_rng(11).integers(1, 6, size=n)]


@functools.lru_cache(maxsize=None)
def triphone(tscale=1.0, lscale=0.1):
    tree, tm = make_model(7, 3, 1, seed=7, num_pdfs=PDFS)
    return chain.AlignModel(tree, tm, tscale, lscale), chain.Lexicon(kaldi_like_lexicon(PRONS), [9, 10])


@functools.lru_cache(maxsize=None)
def numerator_aligner():
    tree, tm = make_model(7, 3, 1, seed=7, num_pdfs=PDFS)
    return chain.MappedAligner.from_models(tm, tree, kaldi_like_lexicon(PRONS1), disambig=[9, 10])


def min_frames(words, hi=8192, model=None):
    """The least T with a path of T frames, by bisection on the compile status (every state of these models has a
    self-loop or is followed by one that has, so the feasible lengths are an interval); both sides of the answer are
    checked."""
    model, lexicon = model or triphone()
    status = lambda T: chain.AlignmentGraphs(model, lexicon, [words], [T]).status[0]    # noqa: E731
    lo = 0
    assert status(hi) == chain.ALIGN_OK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if status(mid) == chain.ALIGN_OK:
            hi = mid
        else:
            lo = mid
    assert status(hi) == chain.ALIGN_OK and (hi == 1 or status(hi - 1) == chain.ALIGN_NO_PATH)
    return hi


@functools.lru_cache(maxsize=None)
def rung(k):
    """(words, T) of rung k: its transcript at the minimum length + 50 frames."""
    n, lo, hi = RUNGS[k]
    words = ladder_words(n)
    return words, min_frames(words) + 50


def assert_rung(k, S):
    _, lo, hi = RUNGS[k]
    assert lo < S <= hi, "rung %d: %d states, wanted %d < S <= %d" % (k, S, lo, hi)
    assert states_per_thread(S) == {1: 4, 2: 8, 3: 16, 4: 32}[k]


def planted(rng, graph, T, pdfs, peak=8.0):
    """A random path of exactly T frames through an exported graph, and log-likelihoods peaked along its pdfs."""
    S = graph["final"].shape[0]
    src, dst = graph["src"], graph["dst"]
    reach = np.zeros((T, S), bool)
    reach[0, dst[src < 0]] = True
    for t in range(1, T):
        ok = (src >= 0) & reach[t - 1, np.maximum(src, 0)]
        reach[t, dst[ok]] = True
    cand = np.flatnonzero(reach[T - 1] & np.isfinite(graph["final"]))
    s = int(rng.choice(cand))
    arcs = []
    for t in range(T - 1, -1, -1):
        ks = np.flatnonzero((dst == s) & ((src < 0) if t == 0 else ((src >= 0) & reach[t - 1, np.maximum(src, 0)])))
        k = int(rng.choice(ks))
        arcs.append(k)
        s = int(src[k])
    arcs = arcs[::-1]
    ll = rng.uniform(-1.0, 0.0, (T, pdfs)).astype(np.float32) - peak
    ll[np.arange(T), graph["pdf"][arcs]] = 0.0
    return ll, graph["tid"][arcs]


@functools.lru_cache(maxsize=None)
def rung_loglikes(k):
    """Noise of deviation 3 with 3.0 added along a planted path.  With T only 50 frames above the minimum a path has to
    move on almost every frame and pays a transition cost each time, while a state that idles in its self-loop does not:
    on noise alone the frame's best state is one that can no longer finish, the best complete path lies a hundred or
    more above it, and every beam below that loses all final states.  The planted bonus (0.3 a frame at ASCALE) brings the
    competition between complete paths inside the beam, so that a binding beam prunes the unpruned winner and
    still ends on another path."""
    g, T = rung_graph(k), rung(k)[1]
    rng = np.random.default_rng(100 + k)
    peaked, _ = planted(rng, g, T, PDFS)
    ll = (3.0 * rng.standard_normal((T, PDFS))).astype(np.float32)
    ll[peaked == 0.0] += np.float32(3.0)
    ll.setflags(write=False)
    return ll


@functools.lru_cache(maxsize=None)
def rung_graph(k):
    """The compiled graph of rung k alone, exported: what the references below run on (the arrays of a graph do not
    depend on the batch it was compiled in)."""
    words, T = rung(k)
    model, lexicon = triphone()
    graphs = chain.AlignmentGraphs(model, lexicon, [words], [T])
    assert graphs.status == [0], graphs.errors
    assert_rung(k, graphs.num_states[0])
    return graphs.export(0)


@functools.lru_cache(maxsize=None)
def viterbi_reference(k, beam):
    """emulate_viterbi of rung k at `beam`, and its trace."""
    trace = {}
    out = emulate_viterbi(rung_graph(k), rung_loglikes(k), ASCALE, beam, trace=trace)
    return out, trace


def differs(a, b):
    """Two emulation results with status 0: another alignment or another cost?"""
    return not np.array_equal(a[1], b[1]) or any(np.float32(x).tobytes() != np.float32(y).tobytes() for x, y in zip(a[2:], b[2:]))


# Phone 5 has the skip topology: as the last phone of a transcript it ends in two final states (state 0 left by the skip,
# state 1 left forwards) that no cost tells apart once the transition scales are zero.
PRONS_TIES = PRONS + [(6, [4, 5], 0.2, None)]


@functools.lru_cache(maxsize=None)
def ties_case():
    """(graphs, T, beams): the rung-1 transcript followed by word 6, compiled with both scales 0."""
    tree, tm = make_model(7, 3, 1, seed=7, num_pdfs=PDFS)
    model, lexicon = chain.AlignModel(tree, tm, 0.0, 0.0), chain.Lexicon(kaldi_like_lexicon(PRONS_TIES), [9, 10])
    words = ladder_words(RUNGS[1][0]) + [6]
    T = min_frames(words, model=(model, lexicon)) + 50
    graphs = chain.AlignmentGraphs(model, lexicon, [words], [T])
    return graphs, T, (1e30, 43.0)        # the second one prunes, and keeps the best path (its margin is 42.3)


@functools.lru_cache(maxsize=None)
def ties_reference(beam):
    graphs, T, _ = ties_case()
    trace = {}
    out = emulate_viterbi(graphs.export(0), np.zeros((T, PDFS), np.float32), ASCALE, beam, trace=trace)
    return out, trace


SCALE_WORDS, SCALE_FRAMES = [3, 5, 4], 60


@functools.lru_cache(maxsize=None)
def scale_range_case(gap):
    """Logits whose frame maximum sits on a pdf the graph uses but no path can be on at that frame -- at frame 0 and at the
    frame nearest the middle that has such a pdf -- `gap` above the frame's largest other logit.  The kernel scales a
    frame by the maximum over the pdfs of all states of the graph, so every live factor of these frames is e^-gap or
    less; the float64 log-domain oracle does not care.  -> dict(words, T, x, outliers [(t, pdf)], want, plain)."""
    words, T = SCALE_WORDS, SCALE_FRAMES
    gs = chain.graph_supervisions(numerator_aligner(), [words], [T], transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0], gs.errors
    g = gs.graphs.export(0)
    x = (2.0 * np.random.default_rng(300).standard_normal((T, PDFS))).astype(np.float32)
    lp, gamma, occ = R.forward_backward(g, x, with_arcs=True)
    used = np.unique(g["pdf"])
    idle = lambda t: [int(q) for q in used if not occ[t, g["pdf"] == q].any()]      # noqa: E731
    middle = next(t for t in sorted(range(1, T - 1), key=lambda t: abs(t - T // 2)) if idle(t))
    outliers = []
    for t in (0, middle):
        q = idle(t)[0]
        x[t, q] = np.delete(x[t], q).max() + np.float32(gap)
        outliers.append((t, q))
    x.setflags(write=False)
    return dict(words=words, T=T, x=x, outliers=outliers, want=R.forward_backward(g, x), plain=(lp, gamma))


@functools.lru_cache(maxsize=None)
def numerator_case(k, bonus=4.0):
    """Rung k for the numerator: (words, T, logits, (log p, gamma) of the float64 oracle).  The logits are noise of
    deviation 2 with `bonus` added along a planted path of T frames.  The bonus is there for the reason rung_loglikes
    gives: at 50 frames above the minimum length, on noise alone, the forward mass sits on states that can no longer
    finish -- the paths that do finish hold e^-479 of the last alpha row at rung 1 -- and the kernel, which works in
    float32 probability space with one scale per frame, has no range for that (bonus = 0 is noise_only_case below).
    With the bonus the largest scaled alpha * beta of a frame never falls below e^-12."""
    words, T = rung(k)
    gs = chain.graph_supervisions(numerator_aligner(), [words], [T], transition_scale=1.0, self_loop_scale=0.1)
    assert gs.status == [0], gs.errors
    assert_rung(k, gs.graphs.num_states[0])
    g = gs.graphs.export(0)
    rng = np.random.default_rng(200 + k)
    peaked, _ = planted(rng, g, T, PDFS)
    x = (2.0 * rng.standard_normal((T, PDFS))).astype(np.float32)
    x[peaked == 0.0] += np.float32(bonus)
    x.setflags(write=False)
    lp, gamma = R.forward_backward(g, x)
    gamma.setflags(write=False)
    return words, T, x, (lp, gamma)


def noise_only_case():
    """Rung 1 without the planted bonus: beyond the float32 range of the kernel; the float64 oracle is at ease."""
    return numerator_case(1, bonus=0.0)
