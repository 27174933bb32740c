"""Lattices for the forward-backward tests (tests/test_gpu_lattice_fb.py) whose frames are wide enough to reach the paths of
pykaldi2_amd/csrc/lattice_fb.hip that the lattices of test_gpu_lattice.py::CASES never reach, the oracle's view of them, and the
error model the posterior tolerances come from -- test infrastructure only, everything here runs on the CPU.

A case is a tuple in the CASES format of test_gpu_lattice.py: words pdfs T seed beam lat_beam ac max_active min_active."""
import functools
import math

import numpy as np

from oracle import lattice_ref as lr
from pykaldi2_amd import synth
# (one copy of the set-up helpers: the module imports without a GPU)
from test_gpu_lattice import CASES, _ali_near_lattice, _ref_graph, _setup

# The limits of lat_fb_alpha_beta_lin (lattice_fb.hip) the cases are built around:
LIN_EMIT_SLOTS = 4 * 512       # kLinEmit * kLinThreads: emitting links of a frame held in registers; the rest take the overflow loop
LIN_EPS_SLOTS = 2 * 512        # kLinEps * kLinThreads: the same for the epsilon links of a frame
LIN_THREADS = 512              # kLinThreads: a frame with more links than this puts a second record into some thread
LDS_FRAME_TOKENS = 19456 // 2  # kFbCap / 2: a frame with more tokens is accumulated in global memory, in the log domain

UNLIMITED = 2 ** 31 - 1
WIDE = {
    # every frame in LDS; 2400 .. 12000 emitting links per frame and 1200 epsilon links in frame 0: both overflow loops run
    "WIDE_A": (1200, 40, 5, 8, 40.0, 30.0, 0.05, UNLIMITED, 200),
    # 1500 epsilon links in frame 0 AND in frame T: the backward recursion starts on an epsilon overflow
    "WIDE_B": (1500, 40, 6, 3, 40.0, 30.0, 0.05, UNLIMITED, 200),
    # frames 3-5 hold more tokens than an LDS half-array: forward linear -> log, backward log -> linear (to_linear), no hook
    "WIDE_C": (2500, 40, 5, 8, 40.0, 30.0, 0.05, UNLIMITED, 200),
    # up to 1842 emitting links in a frame: all four register slots of a thread, no overflow loop
    "WIDE_D": (300, 60, 10, 5, 30.0, 20.0, 0.1, UNLIMITED, 200),
}
MAX_PHONES = {"WIDE_A": 2, "WIDE_B": 2, "WIDE_C": 2, "WIDE_D": 3}


def decode_ref(g, tm, ll, case):
    beam, lb, ac, maxa, mina = case[4:]
    return lr.decode(_ref_graph(g), ll, tm["tid2pdf"], lr.DecoderOptionsRef(beam, lb, maxa, mina, 0.5, ac))


class Case:
    """A decoded case: graph, model, scores, the oracle's lattice and a reference alignment (never modified once made)."""

    def __init__(self, case, max_phones=3, frames=None):
        """frames: only the first `frames` frames of the case's scores (its alignment cut to them)."""
        self.P, self.T = case[1], case[2]
        self.g, self.tm, self.ll, rng = _setup(*case[:4], max_phones=max_phones)
        if frames is not None:
            full = Case(case, max_phones)
            self.T, self.ll, case = frames, self.ll[:frames], case[:2] + (frames,) + case[3:]
        self.case = case
        self.want = decode_ref(self.g, self.tm, self.ll, case)
        self.ali = _ali_near_lattice(rng, self.want, self.P) if frames is None else full.ali[:frames]
        self.A = self.want.arrays()


@functools.lru_cache(maxsize=None)
def wide(name):
    return Case(WIDE[name], MAX_PHONES[name])


@functools.lru_cache(maxsize=None)
def wide_cut(name, frames):
    return Case(WIDE[name], MAX_PHONES[name], frames)


@functools.lru_cache(maxsize=None)
def case(name):
    """WIDE_x, CASESi (test_gpu_lattice.py::CASES[i]) or RANGE_n (the two-branch lattice with X h = n, below)."""
    if name.startswith("CASES"):
        return Case(CASES[int(name[5:])], 3)
    if name.startswith("RANGE_"):
        return range_case(int(name[6:]) / RANGE_H)
    return wide(name)


def settings(name):
    """What the GPU tests run on a case: [(criterion, arguments)], the arguments as the terms_* functions take them."""
    rng_ = name.startswith("RANGE_")
    out = []
    if not name.startswith("CASES"):        # (MMI and posteriors of CASES[:3]: test_gpu_lattice.py, test_gpu_ts.py)
        out += [("mmi", (1.0 if rng_ else 0.2, drop)) for drop in (True, False)]
        out += [("posteriors", (kappa,)) for kappa in ((1.0,) if rng_ else (1.0, 0.2))]
    out += [("mpe", (criterion, osc)) for criterion in ("smbr", "mpfe") for osc in ((True,) if rng_ else (True, False))]
    return out


def oracle(name, criterion, args):
    """-> (value, post[T, P], bound) of the oracle for one setting of a case."""
    c = case(name)
    t2p = c.tm["tid2pdf"]
    if criterion == "mmi":
        v, wp = lr.lattice_mmi(c.want, c.ali, t2p, c.P, 1.0, args[0], args[1])
        return v, wp, post_bound(*terms_mmi(c.want, c.ali, t2p, 1.0, args[0], args[1]), c.T, c.P)
    if criterion == "posteriors":
        t, pdf, g = terms_posteriors(c.want, t2p, 1.0, args[0])
        wp = np.zeros((c.T, c.P))
        np.add.at(wp, (t, pdf), g)             # (tests/ts_ref.py::posteriors: the same sums)
        return lr.lattice_forward_backward(c.want, 1.0, args[0])[0], wp, post_bound(t, pdf, g, c.T, c.P)
    v, wp = lr.lattice_mpe(c.want, c.ali, t2p, c.tm["tid2phone"], c.tm["silence_phones"], c.P, args[0], args[1])
    return v, wp, post_bound(*terms_mpe(c.want, c.ali, c.tm, c.P, args[0], args[1]), c.T, c.P, max(1.0, np.abs(wp).max()))


def frame_counts(A, T):
    """Per frame t = 0 .. T of a lattice's arrays: tokens, emitting links t -> t+1 (0 for frame T), epsilon links inside t."""
    fr = np.asarray(A["tok_frame"])
    src_fr = fr[np.asarray(A["link_src"])]
    eps = np.asarray(A["link_tid"]) == 0
    tokens = np.bincount(fr, minlength=T + 1)
    emitting = np.bincount(src_fr[~eps], minlength=T + 1)
    epsilon = np.bincount(src_fr[eps], minlength=T + 1)
    return tokens, emitting, epsilon


# ----------------------------------------------------------------------------------------------------------------------
# Float64 per-link terms of the three posterior matrices (the oracle's own sums, term by term), and what a float32
# accumulation of them in an arbitrary order -- the device's atomicAdd into a float32 row -- can be off by.
# ----------------------------------------------------------------------------------------------------------------------
def _emitting(A):
    em = np.flatnonzero(np.asarray(A["link_tid"]) > 0)
    return em, np.asarray(A["tok_frame"])[np.asarray(A["link_src"])[em]]


def _gamma(lat, lm_scale, ac_scale):
    tot, alpha, beta, like, order, A = lr.lattice_forward_backward(lat, lm_scale, ac_scale)
    x = alpha[A["link_src"]] + like + beta[A["link_dst"]] - tot
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(np.isfinite(x), np.exp(x), 0.0)
    return A, g


def terms_posteriors(lat, tid2pdf, lm_scale, ac_scale):
    """-> (frame, pdf, term) of every emitting link for the plain posteriors."""
    A, g = _gamma(lat, lm_scale, ac_scale)
    em, t = _emitting(A)
    return t, np.asarray(tid2pdf)[A["link_tid"][em]], g[em]


def terms_mmi(lat, ali, tid2pdf, lm_scale, ac_scale, drop_frames):
    """-> (frame, pdf, term): -gamma of every emitting link of a frame that is not dropped, +1 for its reference."""
    A, g = _gamma(lat, lm_scale, ac_scale)
    em, t = _emitting(A)
    tid = A["link_tid"][em]
    ref = np.asarray(ali)[:lat.T]
    ref_post = np.zeros(lat.T)
    hit = tid == ref[t]
    np.add.at(ref_post, t[hit], g[em][hit])
    live = np.ones(lat.T, bool) if not drop_frames else ref_post != 0.0
    keep = live[t]
    tt = np.concatenate([t[keep], np.flatnonzero(live)])
    pdf = np.concatenate([np.asarray(tid2pdf)[tid[keep]], np.asarray(tid2pdf)[ref[live]]])
    val = np.concatenate([-g[em][keep], np.ones(int(live.sum()))])
    return tt, pdf, val


def terms_mpe(lat, ali, tm, num_pdfs, criterion, one_silence_class):
    """-> (frame, pdf, term) for sMBR / MPFE: a restatement of lattice_mpe's last loop on its own alpha_smbr / beta_smbr
    (recomputed here the same way; checked against lattice_mpe's matrix by the CPU test)."""
    tid2pdf, tid2phone = tm["tid2pdf"], tm["tid2phone"]
    tot, alpha, beta, like, order, A = lr.lattice_forward_backward(lat, 1.0, 1.0)
    sil = set(int(x) for x in tm["silence_phones"])
    nl, nt = like.shape[0], alpha.shape[0]
    acc = np.zeros(nl)
    for l in np.flatnonzero(A["link_tid"] > 0):
        tid, ref = int(A["link_tid"][l]), int(ali[A["tok_frame"][A["link_src"][l]]])
        phone, ref_phone = int(tid2phone[tid]), int(tid2phone[ref])
        phone_sil, both_sil = phone in sil, (phone in sil and ref_phone in sil)
        a, b = (phone, ref_phone) if criterion == "mpfe" else (int(tid2pdf[tid]), int(tid2pdf[ref]))
        acc[l] = float((a == b or both_sil) if one_silence_class else (a == b and not phone_sil))
    a_s, b_s = np.zeros(nt), np.zeros(nt)
    for l in order:
        s, d = A["link_src"][l], A["link_dst"][l]
        a_s[d] += math.exp(alpha[s] + like[l] - alpha[d]) * (a_s[s] + acc[l])
    score = 0.0
    for k in np.flatnonzero(A["tok_final"] != lr.INF):
        score += math.exp(alpha[k] - float(np.float32(A["tok_final"][k])) - tot) * a_s[k]
    for l in reversed(order):
        s, d = A["link_src"][l], A["link_dst"][l]
        if beta[s] != -math.inf and beta[d] != -math.inf:
            b_s[s] += math.exp(beta[d] + like[l] - beta[s]) * (b_s[d] + acc[l])
    em, t = _emitting(A)
    s, d = A["link_src"][em], A["link_dst"][em]
    live = beta[d] != -math.inf
    em, t, s, d = em[live], t[live], s[live], d[live]
    val = np.exp(alpha[s] + like[em] + beta[d] - tot) * (a_s[s] + acc[em] + b_s[d] - score)
    return t, np.asarray(tid2pdf)[A["link_tid"][em]], val


def f32_model_deviation(t, pdf, val, T, num_pdfs, orders=8, seed=0):
    """The largest |float32 accumulation - float64 sum| over the cells of the [T, P] matrix, the terms rounded to float32 and
    added one by one in `orders` random orders."""
    cell = np.asarray(t, np.int64) * num_pdfs + np.asarray(pdf, np.int64)
    exact = np.zeros(T * num_pdfs)
    np.add.at(exact, cell, val)
    rng = np.random.default_rng(seed)
    v32 = np.asarray(val, np.float32)
    worst = 0.0
    for _ in range(orders):
        perm = rng.permutation(cell.shape[0])
        c, v = cell[perm], v32[perm]
        # a stable sort by cell keeps the random order inside every cell; one running float32 sum per cell
        o = np.argsort(c, kind="stable")
        c, v = c[o], v[o]
        acc = np.zeros(T * num_pdfs, np.float32)
        start = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
        rank = np.arange(c.shape[0]) - np.repeat(start, np.diff(np.r_[start, c.shape[0]]))
        by_rank = np.argsort(rank, kind="stable")
        c, v = c[by_rank], v[by_rank]
        cut = np.r_[np.flatnonzero(np.r_[True, rank[by_rank][1:] != rank[by_rank][:-1]]), c.shape[0]]
        for k in range(cut.shape[0] - 1):         # step k: the k-th term of every cell (one per cell), a float32 add
            m = slice(cut[k], cut[k + 1])
            acc[c[m]] = acc[c[m]] + v[m]
        worst = max(worst, float(np.abs(acc.astype(np.float64) - exact).max()))
    return worst


def post_bound(t, pdf, val, T, num_pdfs, scale=1.0):
    """The tolerance of a posterior matrix: max(2e-6, 4 x the float32 model's largest deviation over 8 random link orders)
    -- the factor 4 for the orders the model did not draw --, times `scale` (sMBR / MPFE: max(1, |want|.max()))."""
    return max(2e-6, 4.0 * f32_model_deviation(t, pdf, val, T, num_pdfs)) * scale


# ----------------------------------------------------------------------------------------------------------------------
# Dynamic range: two branches that never merge; B is X h nats behind at frame h and wins by X h at the end.
# ----------------------------------------------------------------------------------------------------------------------
RANGE_T, RANGE_H, RANGE_CHAIN, RANGE_PDFS = 24, 12, 8, 30


def two_branch_graph(chain=RANGE_CHAIN, num_pdfs=RANGE_PDFS):
    """start -> branch A (pdfs 0 .. chain-1) | branch B (pdfs chain .. 2 chain - 1): chains of `chain` states with self-loops and
    forward arcs, each ending in its own final state; the transition-ids of synth.transition_model_arrays (two per pdf: one
    labels the forward arc into a state, the other its self-loop)."""
    tm = synth.transition_model_arrays(num_pdfs)
    t2p = np.asarray(tm["tid2pdf"])
    first = {}
    for tid in range(1, t2p.shape[0]):
        first.setdefault(int(t2p[tid]), []).append(tid)
    src, dst, il, w = [], [], [], []
    n_states = 1 + 2 * chain
    branch_pdfs = []
    for b in range(2):
        pdfs = list(range(b * chain, (b + 1) * chain))
        branch_pdfs.append(pdfs)
        states = [0] + [1 + b * chain + k for k in range(chain)]
        for k in range(chain):
            tids = first[pdfs[k]]
            src.append(states[k]); dst.append(states[k + 1]); il.append(tids[0]); w.append(0.5 + 0.1 * b)      # forward arc
            src.append(states[k + 1]); dst.append(states[k + 1]); il.append(tids[-1]); w.append(0.3)           # self-loop
    final = np.full(n_states, np.inf, np.float32)
    final[chain] = 0.25
    final[2 * chain] = 0.5
    g = dict(num_states=n_states, start=0, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32),
             ilabel=np.asarray(il, np.int32), weight=np.asarray(w, np.float32), final=final)
    return g, tm, branch_pdfs


def two_branch_loglikes(X, branch_pdfs, T=RANGE_T, h=RANGE_H, num_pdfs=RANGE_PDFS, offset=0.0):
    """offset: added to every score (positive: link weights beyond what the linear form takes)."""
    ll = np.full((T, num_pdfs), -3.0 * X, np.float32)
    a, b = branch_pdfs
    ll[:h, a], ll[:h, b] = 0.0, -X
    ll[h:, a], ll[h:, b] = -2.0 * X, 0.0
    return ll + np.float32(offset)


RANGE_DECODE = (30.0, 25.0, 1e-3, UNLIMITED, 200)      # beam, lattice beam, acoustic scale: both branches survive


class RangeCase:
    def __init__(self, X, offset=0.0):
        self.X, self.P, self.T = X, RANGE_PDFS, RANGE_T
        self.g, self.tm, self.branch_pdfs = two_branch_graph()
        self.ll = two_branch_loglikes(X, self.branch_pdfs, offset=offset)
        self.case = (0, RANGE_PDFS, RANGE_T, 0) + RANGE_DECODE
        self.want = decode_ref(self.g, self.tm, self.ll, self.case)
        self.A = self.want.arrays()
        self.ali = _ali_near_lattice(np.random.default_rng(int(X * 8)), self.want, self.P)


@functools.lru_cache(maxsize=None)
def range_case(X, offset=0.0):
    return RangeCase(float(X), float(offset))
