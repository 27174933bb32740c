"""Float64 restatement of the lattice teacher-student criterion (ops.TeacherStudentMMI, pykaldi2_amd/csrc/lattice_rescore.hip)
-- test infrastructure only.  It works on the arrays of a raw state-level lattice (LatticeBatch.export(n), or
LatticeRef.arrays()), with the forward-backward of oracle.lattice_ref:

  rescore          the rescoring rule in float32: ac' = f32(f32(old_scale * ac) - loglike_S[t, pdf]), old_scale 0: -loglike_S
  posteriors       LatticeForwardBackward + Posterior.to_pdf_matrix with no reference alignment
  teacher_student  loss = sum_l gamma_T(l) (like_T(l) - like_S(l)) - tot_T + tot_S = KL(P_T || P_S) over the paths,
                   grad = post_S - post_T = d loss / d loglike_S divided by the acoustic scale
"""
import math

import numpy as np

from oracle import lattice_ref as lr
from pykaldi2_amd import synth

# tests/test_gpu_lattice.py::CASES[:3]: words pdfs T seed beam lat_beam ac max_active min_active
CASES = [
    (6, 12, 8, 0, 30.0, 3.0, 1.0, 2 ** 31 - 1, 200),
    (40, 60, 40, 1, 8.0, 4.0, 0.5, 2 ** 31 - 1, 0),
    (200, 150, 60, 2, 13.0, 7.0, 0.1, 300, 200),
]


def setup(case):
    """-> (graph arcs, transition-model arrays, teacher log-likelihoods, student log-likelihoods) of a case."""
    nw, P, T, seed = case[:4]
    rng = np.random.default_rng(seed)
    g = synth.decoding_graph_arcs(nw, P, seed=seed, max_phones=3)
    tm = synth.transition_model_arrays(P)
    ll_T = (2.0 * rng.standard_normal((T, P))).astype(np.float32)
    return g, tm, ll_T, student_loglikes(T, P, seed)


def student_loglikes(T, P, seed):
    return (2.0 * np.random.default_rng(100 + seed).standard_normal((T, P))).astype(np.float32)


def decode_ref(case):
    """The oracle's lattice of a case as export arrays (with start_tok and T)."""
    nw, P, T, seed, beam, lb, ac, maxa, mina = case
    g, tm, ll_T, _ = setup(case)
    ref = lr.DecodeGraphRef(g["num_states"], g["start"], g["src"], g["dst"], g["ilabel"], g["weight"], g["final"])
    lat = lr.decode(ref, ll_T, tm["tid2pdf"], lr.DecoderOptionsRef(beam, lb, maxa, mina, 0.5, ac))
    A = lat.arrays()
    A["start_tok"], A["T"] = lat.start_tok, lat.T
    return A


class ArrayLattice:
    """What oracle.lattice_ref.lattice_forward_backward reads of a lattice: arrays(), T, start_tok."""

    def __init__(self, A, link_ac=None):
        self._A = {k: v for k, v in A.items() if k not in ("start_tok", "T")}
        if link_ac is not None:
            self._A["link_ac"] = np.asarray(link_ac, np.float32)
        fr = np.asarray(A["tok_frame"])
        self.T = int(A["T"]) if "T" in A else int(fr.max())
        if "start_tok" in A:
            self.start_tok = int(A["start_tok"])
        else:      # the frame-0 token no link enters
            indeg = np.bincount(np.asarray(A["link_dst"]), minlength=fr.shape[0])
            self.start_tok = int(np.flatnonzero((fr == 0) & (indeg == 0))[0])

    def arrays(self):
        return self._A


def rescore(A, loglikes_S, tid2pdf, old_acoustic_scale=0.0):
    """The rescored link_ac (float32): emitting links by the rule, epsilon links as they are."""
    ac = np.asarray(A["link_ac"], np.float32).copy()
    tid = np.asarray(A["link_tid"])
    em = tid > 0
    t = np.asarray(A["tok_frame"])[np.asarray(A["link_src"])[em]]
    x = np.asarray(loglikes_S, np.float32)[t, np.asarray(tid2pdf)[tid[em]]]
    if old_acoustic_scale == 0:
        ac[em] = -x
    else:
        kept = (np.float32(old_acoustic_scale) * ac[em]).astype(np.float32)
        ac[em] = (kept - x).astype(np.float32)
    return ac


def _link_posteriors(lat, lm_scale, ac_scale):
    tot, alpha, beta, like, order, A = lr.lattice_forward_backward(lat, lm_scale, ac_scale)
    gamma = np.zeros(like.shape[0])
    for l in range(like.shape[0]):
        x = alpha[A["link_src"][l]] + like[l] + beta[A["link_dst"][l]] - tot
        gamma[l] = math.exp(x) if x > -math.inf else 0.0
    return tot, gamma, like


def _pdf_matrix(A, gamma, tid2pdf, T, P):
    post = np.zeros((T, P))
    for l in np.flatnonzero(np.asarray(A["link_tid"]) > 0):
        post[A["tok_frame"][A["link_src"][l]], tid2pdf[A["link_tid"][l]]] += gamma[l]
    return post


def posteriors(A, tid2pdf, num_pdfs, lm_scale=1.0, acoustic_scale=1.0):
    """-> (tot, post[T, P])."""
    lat = ArrayLattice(A)
    tot, gamma, _ = _link_posteriors(lat, lm_scale, acoustic_scale)
    return tot, _pdf_matrix(lat.arrays(), gamma, tid2pdf, lat.T, num_pdfs)


def teacher_student(A, loglikes_S, tid2pdf, num_pdfs, lm_scale=1.0, acoustic_scale=1.0, old_acoustic_scale=0.0):
    """-> dict(post_T, post_S, tot_T, tot_S, loss, grad, link_ac)."""
    lat_T = ArrayLattice(A)
    ac_S = rescore(A, loglikes_S, tid2pdf, old_acoustic_scale)
    lat_S = ArrayLattice(A, ac_S)
    tot_T, g_T, like_T = _link_posteriors(lat_T, lm_scale, acoustic_scale)
    tot_S, g_S, like_S = _link_posteriors(lat_S, lm_scale, acoustic_scale)
    live = g_T > 0.0
    loss = float(np.sum(g_T[live] * (like_T[live] - like_S[live]))) - tot_T + tot_S
    post_T = _pdf_matrix(lat_T.arrays(), g_T, tid2pdf, lat_T.T, num_pdfs)
    post_S = _pdf_matrix(lat_S.arrays(), g_S, tid2pdf, lat_T.T, num_pdfs)
    return dict(post_T=post_T, post_S=post_S, tot_T=tot_T, tot_S=tot_S, loss=loss, grad=post_S - post_T, link_ac=ac_S)


def path_kl(A, loglikes_S, tid2pdf, lm_scale=1.0, acoustic_scale=1.0, old_acoustic_scale=0.0):
    """KL(P_T || P_S) from the distributions over every complete path of a tiny lattice (brute force)."""
    lat = ArrayLattice(A)
    B = lat.arrays()
    ac_S = rescore(A, loglikes_S, tid2pdf, old_acoustic_scale)
    f = lambda scale, v: float(np.float32(scale * float(v)))
    outs = {}
    for l in range(B["link_src"].shape[0]):
        outs.setdefault(int(B["link_src"][l]), []).append(l)
    paths = []

    def walk(k, a, b):
        if len(paths) > 200000:
            raise RuntimeError("too many paths")
        if B["tok_final"][k] != lr.INF:
            fin = f(lm_scale, B["tok_final"][k])
            paths.append((a - fin, b - fin))
        for l in outs.get(k, []):
            gr = f(lm_scale, B["link_graph"][l])
            walk(int(B["link_dst"][l]), a - (gr + f(acoustic_scale, B["link_ac"][l])), b - (gr + f(acoustic_scale, ac_S[l])))

    walk(lat.start_tok, 0.0, 0.0)
    a, b = np.array([p[0] for p in paths]), np.array([p[1] for p in paths])
    la = a - (a.max() + math.log(np.exp(a - a.max()).sum()))
    lb = b - (b.max() + math.log(np.exp(b - b.max()).sum()))
    return float(np.sum(np.exp(la) * (la - lb))), len(paths)
