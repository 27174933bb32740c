"""Restatement of the frequency permutation aligner -- TEST INFRASTRUCTURE ONLY (tests/ and tools/ import
it; the product path never does).  The reference project has no such stage: this numpy float64 text is the oracle.

For one utterance with masks lam (K, N, F), 2 <= K <= 4; every sum is float64 in ascending index order, every stored vector
is rounded once to float32:

  pearson(v)  (v - mean v) / max(||v - mean v||_2, 1e-10)
  features    u[f][k] = pearson(lam[k, :, f])
  best(S)     the permutation p maximising sum_a S[a][p[a]]: the K! candidates in lexicographic order, the first maximum
  tree        level 0: one group per bin (centroid u[f], weight 1).  A level merges the neighbours (2j, 2j + 1):
              S[a][b] = <cL[a], cR[b]>, p = best(S), every bin of the right group gets pi_f <- pi_f o p
              (new pi_f[a] = old pi_f[p[a]]), centroid pearson(wL cL[a] + wR cR[p[a]]), weight wL + wR; a last odd group
              passes up unchanged
  refinement  `refine` rounds: c[a] = pearson(sum_f u[f][pi_f[a]]); per bin S[a][b] = <c[a], u[f][pi_f[b]]>, p = best(S),
              pi_f <- pi_f o p; margin[f] = the best score - the second best, in the last round
  noise last  (with R): q[a] = sum_f ||R||_F^2 / (Re tr R)^2 of R[pi_f[a]][f] over the bins where it is finite; the stream
              with the smallest q moves to position K - 1 (a tie keeps the first), the others keep their order

`dtype=np.float32` is the float32 mode: the scores, means and norms are computed in float32 instead of float64 (the
features and centroids are float32 vectors in both modes).  Its margins against the float64 ones give the tolerance of the
device kernel's margin (4 x): `python tests/perm_align_ref.py` prints them, and the mask errors of the two
blind scenes.
"""
import itertools

import numpy as np

import cgmm_ref

KS, NS, FS = (2, 3, 4), (64, 98, 200), (17, 33, 257)        # the scrambled cases of the host test
GPU_KS, GPU_FS, GPU_NS = (2, 3, 4), (1, 2, 17, 33, 257), (1, 31, 64, 65, 200)
BLIND = ((4, 98, 17, 2, 1), (7, 200, 33, 2, 2))              # (C, N, F, S, seed)
BLIND_ITERS = 20


def _sum(x, dtype=np.float64):
    """the sum over the last axis in ascending index order"""
    x = np.asarray(x, dtype)
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], dtype)
    return np.cumsum(x, axis=-1, dtype=dtype)[..., -1]


def pearson(v, dtype=np.float64):
    """over the last axis; float32 result"""
    v = np.asarray(v, dtype)
    d = (v - (_sum(v, dtype) / dtype(v.shape[-1]))[..., None]).astype(dtype)
    den = np.maximum(np.sqrt(_sum(d * d, dtype)), dtype(1e-10))
    return (d / den[..., None]).astype(np.float32)


def features(lam):
    """(K, N, F) -> float32 (F, K, N)"""
    return pearson(np.asarray(lam, np.float32).astype(np.float64).transpose(2, 0, 1))


def perms(K):
    return np.array(list(itertools.permutations(range(K))))


def best(S):
    """S (..., K, K) -> (p (..., K), top, second): the first maximum in lexicographic order"""
    K = S.shape[-1]
    P = perms(K)
    score = S[..., 0, P[:, 0]]
    for a in range(1, K):
        score = score + S[..., a, P[:, a]]
    i = np.argmax(score, axis=-1)
    top = np.take_along_axis(score, i[..., None], -1)[..., 0]
    rest = score.copy()
    np.put_along_axis(rest, i[..., None], -np.inf, -1)
    return P[i], top, rest.max(axis=-1)


def _scores(a, b, dtype):
    """a (..., K, N), b (..., K, N) -> (..., K, K) of <a[i], b[j]>"""
    return _sum(a.astype(dtype)[..., :, None, :] * b.astype(dtype)[..., None, :, :], dtype)


def align(lam, R=None, refine=3, noise_last=True, dtype=np.float64, tree=True):
    """dict(perm (F, K) int, margin (F,), masks, noise (the stream moved last, or None), q)"""
    lam = np.asarray(lam, np.float32)
    K, N, F = lam.shape
    u = features(lam)
    pi = np.tile(np.arange(K), (F, 1))
    if tree:
        cent, weight, first, level = u, np.ones(F), np.arange(F), 0
        while len(cent) > 1:
            G = len(cent)
            nc, nw, nf = [], [], []
            for j in range(0, G - 1, 2):
                S = _scores(cent[j], cent[j + 1], dtype)
                p = best(S.astype(np.float64))[0]
                lo, hi = first[j + 1], (first[j + 2] if j + 2 < G else F)
                pi[lo:hi] = pi[lo:hi][:, p]
                nc.append(pearson(dtype(weight[j]) * cent[j].astype(dtype) + dtype(weight[j + 1]) * cent[j + 1][p].astype(dtype),
                                  dtype))
                nw.append(weight[j] + weight[j + 1])
                nf.append(first[j])
            if G % 2:
                nc.append(cent[G - 1]); nw.append(weight[G - 1]); nf.append(first[G - 1])
            cent, weight, first, level = np.stack(nc), np.array(nw), np.array(nf), level + 1
    margin = np.zeros(F)
    for _ in range(refine):
        up = np.take_along_axis(u, pi[:, :, None], 1)                     # (F, K, N): u[f][pi_f[a]]
        c = pearson(_sum(up.astype(dtype).transpose(1, 2, 0), dtype), dtype)        # (K, N)
        S = _scores(np.broadcast_to(c, up.shape), up, dtype)
        p, top, second = best(S.astype(np.float64))
        pi = np.take_along_axis(pi, p, 1)
        margin = top - second
    noise, q = None, None
    if R is not None and noise_last:
        pur = cgmm_ref.purity(R)                                          # (K, F)
        pp = np.take_along_axis(pur, pi.T, 0)                             # (K, F): purity of R[pi_f[a]][f]
        q = np.array([_sum(np.where(np.isfinite(pp[a]), pp[a], 0.0)) for a in range(K)])
        noise = int(np.argmin(q))
        order = [a for a in range(K) if a != noise] + [noise]
        pi = pi[:, order]
    return dict(perm=pi, margin=margin, masks=gather(lam, pi), noise=noise, q=q)


def gather(x, perm):
    """x (K, N, F) or (K, F, ...) over bins -> out[a, ..., f] = x[perm[f][a], ..., f]"""
    x = np.asarray(x)
    out = np.empty_like(x)
    K = x.shape[0]
    if x.ndim == 3 and x.shape[2] == perm.shape[0] and not np.iscomplexobj(x):
        for a in range(K):
            out[a] = np.take_along_axis(x, perm[None, None, :, a], 0)[0]
        return out
    for a in range(K):                                                    # (K, F, ...)
        out[a] = x[perm[:, a], np.arange(perm.shape[0])]
    return out


def gather_state(R, la, perm):
    """R (K, F, C, C), la (K, F) gathered by perm (F, K)"""
    f = np.arange(perm.shape[0])
    return np.stack([R[perm[:, a], f] for a in range(perm.shape[1])]), np.stack([la[perm[:, a], f] for a in range(perm.shape[1])])


def activity(r, N, S):
    """(S, N) bool: per speaker on-runs of randint(10, 30) frames separated by randint(8, 24), starting at randint(0, 12)"""
    act = np.zeros((S, N), bool)
    for s in range(S):
        t = r.randint(0, 12)
        while t < N:
            n = r.randint(10, 30)
            act[s, t:t + n] = True
            t += n + r.randint(8, 24)
    return act


def scrambled(K, N, F, seed):
    """(lam (K, N, F) float32, truth (F, K) int): K - 1 speakers with on/off activity (each silent on at least a quarter of
    the frames) and a noise class, soft masks with a seeded jitter, the classes of every bin in a random order:
    lam[k, :, f] = clean[truth[f][k], :, f]."""
    r = np.random.RandomState(1000 * K + N + F + seed)
    while True:
        act = activity(r, N, K - 1)
        if (act.mean(axis=1) <= 0.75).all() and (act.mean(axis=1) >= 0.2).all() and \
                all((act[i] != act[j]).mean() > 0.2 for i in range(K - 1) for j in range(i)):
            break
    level = np.concatenate([np.where(act, 3.0, 0.05), np.ones((1, N))])[:, :, None] * r.uniform(0.5, 1.5, (K, N, F))
    clean = (level / level.sum(axis=0, keepdims=True)).astype(np.float32)
    truth = np.stack([r.permutation(K) for _ in range(F)])
    return gather(clean, truth), truth


def consistent(perm, truth):
    """whether pi_f o truth_f^-1 ... i.e. the aligned stream a is the same clean class in every bin: truth[f][perm[f][a]]"""
    g = np.take_along_axis(truth, perm, 1)
    return (g == g[0]).all(axis=1)


def gpu_case(K, N, F):
    """The aligner's GPU cases: scrambled masks, R (K, F, C, C) complex64 with one flat (noise-like) class per bin and
    log_alpha (K, F), scrambled the same way.  C = 2 + (K + F) % 3."""
    lam, truth = scrambled(K, max(N, 1), F, 7) if N >= 40 else _small(K, N, F)
    r = np.random.RandomState(K * 7 + N * 3 + F)
    C = 2 + (K + F) % 3
    d = (r.standard_normal((K, F, C)) + 1j * r.standard_normal((K, F, C)))
    R = d[..., :, None] * np.conj(d[..., None, :]) + 0.05 * np.eye(C)
    R[K - 1] = np.eye(C) * r.uniform(0.5, 2.0, (F, 1, 1)) + 0.05 * R[K - 1]
    la = np.log(r.dirichlet(np.ones(K), F).T)
    f = np.arange(F)
    R = np.stack([R[truth[:, k], f] for k in range(K)]).astype(np.complex64)
    la = np.stack([la[truth[:, k], f] for k in range(K)]).astype(np.float32)
    return lam, R, la, truth


def _small(K, N, F):
    r = np.random.RandomState(K + 10 * N + 100 * F)
    lam = r.uniform(0.05, 1.0, (K, N, F))
    lam = (lam / lam.sum(axis=0, keepdims=True)).astype(np.float32)
    return lam, np.tile(np.arange(K), (F, 1))


def blind_scene(C, N, F, S, seed):
    """(Y (C, N, F) complex64, images (S, C, N, F) complex128): S rank-one speakers with speech-like on/off activity in
    white noise 10 dB below them."""
    r = np.random.RandomState(seed)

    def cplx(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2)
    Y = 10 ** (-10 / 20) * cplx(C, N, F)
    img = []
    for s in range(S):
        d = r.uniform(0.7, 1.3, (C, F)) * np.exp(1j * r.uniform(0, 2 * np.pi, (C, F)))
        t, on = r.randint(0, 12), np.zeros(N, bool)
        while t < N:
            n = r.randint(10, 30)
            on[t:t + n] = True
            t += n + r.randint(8, 24)
        src = cplx(N, F) * (r.uniform(0, 1, (N, F)) < 0.5) * on[:, None]
        img.append(d[:, None, :] * src[None])
        Y = Y + img[-1]
    return Y.astype(np.complex64), np.stack(img)


def random_init(K, N, F, seed, index=0):
    """cgmm_masks(init='random', seed): utterance `index` of the call"""
    x = np.random.default_rng([seed, index]).random((K, N, F), np.float32) + np.float32(0.05)
    return (x / x.sum(axis=0, keepdims=True)).astype(np.float32)


_BLIND = {}


def blind(case, dtype=np.float64):
    """The whole chain on a blind scene, computed once per process: dict(Y, img, em (cgmm_ref.em's), al (align's), R, la)"""
    key = (case, dtype)
    if key not in _BLIND:
        C, N, F, S, seed = case
        Y, img = blind_scene(C, N, F, S, seed)
        e = cgmm_ref.em(Y, BLIND_ITERS, random_init(S + 1, N, F, 0), order="keep", dtype=dtype)
        al = align(e["masks"].astype(np.float32), e["R"], dtype=dtype)
        R, la = gather_state(e["R"], e["la"], al["perm"])
        _BLIND[key] = dict(Y=Y, img=img, em=e, al=al, R=R, la=la)
    return _BLIND[key]


def si_sdr(est, ref):
    est, ref = np.asarray(est).ravel(), np.asarray(ref).ravel()
    a = np.vdot(ref, est) / np.vdot(ref, ref)
    return float(10 * np.log10(np.sum(np.abs(a * ref) ** 2) / np.sum(np.abs(est - a * ref) ** 2)))


def separate(Y, masks, S, ref=0, diag_load=1e-3):
    """S spectra (N, F): speaker s from mask s against 1 - mask s, MVDR in float64"""
    import beamform_ref
    out = []
    for s in range(S):
        phi = beamform_ref.covariance(Y, masks[s:s + 1], True)
        w, _ = beamform_ref.mvdr_weights(phi[0], phi[1], ref, diag_load)
        out.append(beamform_ref.apply(Y, w))
    return out


def stream_gains(Y, img, streams, ref=0):
    """per speaker, over the assignment of streams to speakers that is best in total: SI-SDR of its stream against its image
    at the reference channel minus the reference channel's own.  (gains, assignment)"""
    S = len(streams)
    own = [si_sdr(Y[ref], img[s, ref]) for s in range(S)]
    bestp, bestg = None, None
    for p in itertools.permutations(range(S)):
        g = [si_sdr(streams[p[s]], img[s, ref]) - own[s] for s in range(S)]
        if bestg is None or sum(g) > sum(bestg):
            bestp, bestg = p, g
    return bestg, bestp


def float32_margin_error(K, N, F):
    lam = gpu_case(K, N, F)[0]
    a, b = align(lam), align(lam, dtype=np.float32)
    same = (a["perm"] == b["perm"]).all(axis=1)
    return float(np.abs(a["margin"] - b["margin"])[same].max()) if same.any() else 0.0


if __name__ == "__main__":
    worst = 0.0
    for K in GPU_KS:
        for F in GPU_FS:
            for N in GPU_NS:
                e = float32_margin_error(K, N, F)
                worst = max(worst, e)
                print("k%d_f%d_n%d margin %.2e" % (K, F, N, e))
    print("largest margin error of the float32 mode: %.2e" % worst)
    for case in BLIND:
        w, g = blind(case), blind(case, np.float32)
        ok = w["al"]["margin"] >= 0.02
        same = (w["al"]["perm"] == g["al"]["perm"]).all(axis=1)
        print("blind", case, "masks %.2e (bins with the same order: %d of %d; margin >= 0.02: %d; min margin %.3f; q %s)"
              % (np.abs(w["al"]["masks"] - g["al"]["masks"])[:, :, same].max(), same.sum(), len(same), ok.sum(),
                 w["al"]["margin"].min(), np.round(w["al"]["q"], 2)))
        S = case[3]
        gains, _ = stream_gains(w["Y"], w["img"], separate(w["Y"], w["al"]["masks"], S))
        print("blind", case, "SI-SDR gain per speaker over channel 0: " + " ".join("%.2f dB" % x for x in gains))
