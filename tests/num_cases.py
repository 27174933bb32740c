"""Supervision FSTs for the numerator tests (tests/test_gpu_chain_num.py) that reach the branches of
pykaldi2_amd/csrc/chain_num.h the alignment-built supervisions of test_gpu_chain.py never reach (wide frames, weighted arcs,
several final states, the unstaged accessors, the state limit), the oracle's view of them, and the float32 restatement of
the kernel's recursion the tolerances come from -- test infrastructure only, everything here runs on the CPU."""
import functools

import numpy as np

from oracle import chain_ref as R

P = 40

# The limits of chain_num.h / chain_num.hip the cases are built around:
NUM_MAX_STATES = 18000          # kNumMaxStates: alpha and beta of a sequence are 2 * 18000 floats of LDS
STAGE_MAX_LDS = 128 * 1024      # num_compute: frame table and arc arrays are copied into LDS when everything fits this
DPP_ARCS = 16                   # num_frame_sum: a frame of at most 16 arcs is summed by the 16-lane DPP reduction
WAVE = 64                       # a frame with more arcs than lanes: the lane-strided loops take a second round
REG_ARCS = {64: 4 * 64, 256: 4 * 256}   # num_fwd_bwd_body<THREADS>: arcs of a frame kept in registers; the rest are recomputed

# The bounds of the GPU tests: 4 x the largest error of scaled32() against the float64 oracle over the cases of NAMED (the rule of
# tests/test_gpu_fft.py), measured on the CPU by test_num_cases.py::test_restatement_against_oracle, which prints them and
# asserts that they still hold.  Measured (worst cases first):
#   posteriors, absolute on a row that sums to 1:  6.82e-7 (long), 6.21e-7 (max_states), 3.26e-7 (too_many_states)
#   log p_num, relative to max(1, |lp|):           6.32e-7 (too_many_states), 1.78e-7 (max_states), 6.15e-8 (one_frame)
# (with the two-wave body's __expf modelled -- x * log2(e) rounded to float32, then exp2 -- the staged cases, the only ones
# that body runs, give at most 5.43e-7 (long_staged) and 6.21e-8: inside the same bounds, so the plain restatement stands)
POST_BOUND = 2.8e-6
LP_BOUND = 2.6e-6


def default_states(widths):
    """States per layer for a list of arcs per frame: half of what the arc counts on either side allow, 1 at the start."""
    T = len(widths)
    return [1] + [max(1, min(widths[t - 1], widths[t]) // 2) for t in range(1, T)] + [max(1, widths[T - 1] // 2)]


def layered(rng, widths, states, P, wmax=2.0, dead_ends=0, unreachable=0):
    """A chain.Supervision dict (with state_time for R.NumFstRef): layer t holds states[t] states (states[0] == 1: the initial
    state), widths[t] >= max(states[t], states[t + 1]) arcs go from layer t to layer t + 1 -- the first states[t] sources and
    the first states[t + 1] destinations enumerate the layer, the rest are random, both lists are shuffled, so every state
    has an arc in and an arc out --, random pdfs, arc weights uniform in [0, wmax], every state of the last layer final with a
    random final weight.
    dead_ends / unreachable (needs T >= 2): that many further states, dealt round-robin to the layers 1 .. T-1, that are
    entered (two arcs each) but have no way on / that have two arcs out but are never entered; no path through them reaches
    a final state, so the posterior of their arcs is exactly 0.  Their ids are returned as `dead_states` / `unreachable_states`."""
    T = len(widths)
    assert len(states) == T + 1 and states[0] == 1
    extra_dead = [[] for _ in range(T + 1)]
    extra_unre = [[] for _ in range(T + 1)]
    if dead_ends or unreachable:
        assert T >= 2
        for k in range(dead_ends):
            extra_dead[1 + k % (T - 1)].append(k)
        for k in range(unreachable):
            extra_unre[1 + (k + 1) % (T - 1)].append(k)
    count = [states[t] + len(extra_dead[t]) + len(extra_unre[t]) for t in range(T + 1)]
    first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    src, dst, offsets = [], [], [0]
    dead_ids, unre_ids = [], []
    for t in range(T):
        ns, nd, w = states[t], states[t + 1], widths[t]
        assert w >= max(ns, nd), (t, w, ns, nd)
        s = np.concatenate([np.arange(ns), rng.integers(0, ns, size=w - ns)])
        d = np.concatenate([np.arange(nd), rng.integers(0, nd, size=w - nd)])
        rng.shuffle(s)
        rng.shuffle(d)
        s, d = s + first[t], d + first[t + 1]
        # arcs into the dead ends of layer t + 1, arcs out of the never-entered states of layer t
        for j in range(len(extra_dead[t + 1])):
            s = np.concatenate([s, first[t] + rng.integers(0, ns, size=2)])
            d = np.concatenate([d, np.full(2, first[t + 1] + nd + j)])
        for j in range(len(extra_unre[t])):
            s = np.concatenate([s, np.full(2, first[t] + ns + len(extra_dead[t]) + j)])
            d = np.concatenate([d, first[t + 1] + rng.integers(0, nd, size=2)])
        perm = rng.permutation(s.shape[0])
        src.append(s[perm])
        dst.append(d[perm])
        offsets.append(offsets[-1] + s.shape[0])
    for t in range(T + 1):
        dead_ids += [first[t] + states[t] + j for j in range(len(extra_dead[t]))]
        unre_ids += [first[t] + states[t] + len(extra_dead[t]) + j for j in range(len(extra_unre[t]))]
    src, dst = np.concatenate(src), np.concatenate(dst)
    A = src.shape[0]
    return dict(num_states=int(first[-1]), frames=T, src=src.astype(np.int32), dst=dst.astype(np.int32),
                pdf=rng.integers(0, P, size=A).astype(np.int32), weight=rng.uniform(0.0, wmax, size=A).astype(np.float32),
                frame_offsets=np.asarray(offsets, dtype=np.int32),
                state_time=np.repeat(np.arange(T + 1), count).astype(np.int32),
                final_states=(first[T] + np.arange(states[T])).astype(np.int32),
                final_weights=rng.uniform(0.0, wmax, size=states[T]).astype(np.float32),
                dead_states=np.asarray(dead_ids, dtype=np.int32), unreachable_states=np.asarray(unre_ids, dtype=np.int32))


EDGES = [1, 16, 17, 64, 65, 257, 300, 1025, 1100, 33, 16, 4]
# name -> widths, states (None: default_states), logit scale, entry set to 45.0, (dead ends, unreachable states)
CASES = {
    "one_frame": ([3], [1, 2], 3.0, False, (0, 0)),
    "narrow": ([1, 2, 3] + [5] * 20, None, 3.0, False, (0, 0)),
    # 2898 arcs, staged; frames on both sides of 16 | 17, 64 | 65, 4 * 64 and 4 * 256 arcs
    "edges": (EDGES, None, 3.0, False, (0, 0)),
    "peaked": (EDGES, None, 12.0, True, (0, 0)),
    # scale drift over 602 frames (7205 arcs: unstaged)
    "long": ([1, 4] + [12] * 600, None, 6.0, False, (0, 0)),
    # 7961 arcs: 5 * arcs * 4 B exceed the staged limit
    "unstaged": ([1, 40] + [180] * 36 + [1100, 300, 40], None, 3.0, False, (0, 0)),
    "max_states": ([8999, 8999, 8999], [1, 8999, 8999, 1], 3.0, False, (0, 0)),
    "too_many_states": ([9000, 9000, 8999], [1, 9000, 8999, 1], 3.0, False, (0, 0)),
    "dead_ends": ([1, 4, 9, 18, 20, 70, 30, 12, 6], None, 3.0, False, (5, 4)),
    # not among NAMED (the bounds do not come from them): for the carriers the cases above cannot reach
    # the 602 frames again with half the arcs (3605: staged), for the two-wave body
    "long_staged": ([1, 4] + [6] * 600, None, 6.0, False, (0, 0)),
    # both sides of 16 | 17 and 64 | 65 in 200 arcs (4.7 KB staged): what fits a small persistent table (the two-wave body has no
    # other threshold)
    "edges_small": ([1, 16, 17, 64, 65, 33, 4], None, 3.0, False, (0, 0)),
}
NAMED = ["one_frame", "narrow", "edges", "peaked", "long", "unstaged", "max_states", "too_many_states", "dead_ends"]


class Case:
    """A generated case: the Supervision dict, float32 logits [T, P] and the oracle's view of the FST (never modified)."""

    def __init__(self, name, seed):
        widths, states, scale, spike, (dead, unre) = CASES[name]
        rng = np.random.default_rng([sorted(CASES).index(name), seed])
        self.name, self.widths = name, list(widths)
        self.states = list(states) if states is not None else default_states(widths)
        self.fst = layered(rng, self.widths, self.states, P, dead_ends=dead, unreachable=unre)
        self.T = len(widths)
        self.logits = rng.normal(0.0, scale, size=(self.T, P)).astype(np.float32)
        if spike:
            self.logits[self.T // 2, 7] = 45.0
        f = self.fst
        self.ref = R.NumFstRef(f["num_states"], f["src"], f["dst"], f["pdf"], f["weight"], f["final_states"], f["final_weights"],
                               f["state_time"])
        self.arcs = int(f["src"].shape[0])
        self.frame_arcs = np.diff(f["frame_offsets"])


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    return Case(name, seed)


@functools.lru_cache(maxsize=None)
def oracle(name, seed=0):
    """-> (log p_num, posteriors [T, P]) of the float64 oracle."""
    c = case(name, seed)
    return R.num_forward_backward(c.logits.astype(np.float64), c.ref)


def staged_lds_bytes(cases):
    """LDS the staged numerator of a batch asks for (num_compute): alpha, beta and scratch by the largest state count,
    frame tables by the longest sequence, arc arrays by the sequence with the most arcs."""
    ns = max(c.fst["num_states"] for c in cases)
    return 4 * (2 * ns + 8 + 2 * max(c.T for c in cases) + 2 + 5 * max(c.arcs for c in cases))


def is_staged(cases):
    return staged_lds_bytes(cases) <= STAGE_MAX_LDS


def scaled32(logits, fst, fast_exp=False):
    """The probability-space recursion of chain_num.h in float32 numpy: per-frame max shift, per-frame renormalisation, log p
    accumulated in float64 from m + log z, each frame's posteriors normalised by their own sum.  The sums run in numpy's
    orders, not the device's: the model of an arbitrary order; log p is rounded to float32 at the end, as stored.  fast_exp: exp as the two-wave body's __expf forms it, the
    product x * log2(e) rounded to float32, then exp2.  -> (log p, posteriors [T, P] float32, smallest frame sum z)"""
    f32 = np.float32
    T, npdf = logits.shape
    src, dst, pdf = (np.asarray(fst[k], np.int64) for k in ("src", "dst", "pdf"))
    off = np.asarray(fst["frame_offsets"], np.int64)
    fs = np.asarray(fst["final_states"], np.int64)

    def exp32(x):
        x = np.asarray(x, f32)
        if fast_exp:
            return np.exp2((x * f32(1.4426950408889634)).astype(f32)).astype(f32)
        return np.exp(x).astype(f32)

    frame = np.repeat(np.arange(T), np.diff(off))
    score = (np.asarray(logits, f32)[frame, pdf] - np.asarray(fst["weight"], f32)).astype(f32)
    e = np.empty_like(score)
    fmax = np.empty(T, f32)
    for t in range(T):
        lo, hi = off[t], off[t + 1]
        fmax[t] = score[lo:hi].max()
        e[lo:hi] = exp32(score[lo:hi] - fmax[t])
    ef = exp32(-np.asarray(fst["final_weights"], f32))
    al = np.zeros(fst["num_states"], f32)
    al[0] = 1.0
    inv_prev, lp, zmin = f32(1.0), 0.0, np.inf
    for t in range(T):
        lo, hi = off[t], off[t + 1]
        v = (al[src[lo:hi]] * inv_prev * e[lo:hi]).astype(f32)
        np.add.at(al, dst[lo:hi], v)
        z = v.sum(dtype=f32)
        zmin = min(zmin, float(z))
        lp += float(fmax[t]) + np.log(float(z))
        inv_prev = f32(1.0) / z
    zf = (al[fs] * inv_prev * ef).astype(f32).sum(dtype=f32)
    lp += np.log(float(zf))
    be = np.zeros(fst["num_states"], f32)
    be[fs] = ef
    post = np.zeros((T, npdf), f32)
    inv_prev = f32(1.0)
    for t in range(T - 1, -1, -1):
        lo, hi = off[t], off[t + 1]
        u = (e[lo:hi] * be[dst[lo:hi]] * inv_prev).astype(f32)
        np.add.at(be, src[lo:hi], u)
        q = (al[src[lo:hi]] * u).astype(f32)
        zq, zb = q.sum(dtype=f32), u.sum(dtype=f32)
        zmin = min(zmin, float(zq), float(zb))
        np.add.at(post[t], pdf[lo:hi], (q * (f32(1.0) / zq)).astype(f32))
        inv_prev = f32(1.0) / zb
    return float(f32(lp)), post, zmin      # (num_lp is a float32 array)


def restatement_errors(name, seed=0, fast_exp=False):
    """-> (largest posterior error, |lp error| / max(1, |lp|), smallest frame sum) of scaled32 against the oracle."""
    c = case(name, seed)
    lp, post = oracle(name, seed)
    lp32, post32, zmin = scaled32(c.logits, c.fst, fast_exp)
    return float(np.abs(post32.astype(np.float64) - post).max()), abs(lp32 - lp) / max(1.0, abs(lp)), zmin
