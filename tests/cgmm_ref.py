"""Restatement of the cGMM mask estimator -- TEST INFRASTRUCTURE ONLY (tests/ and tools/ import it; the
product path never does).  The reference project has no such estimator: this numpy float64 text is the oracle.

For one utterance with spectrum Y (C, N, F) complex, K classes and an activity a (K, N) >= 0 (None: all ones), per bin f:

  init        without masks (K = 2): R_0 = sum_t y y^H / N, R_1 = (Re tr R_0 / C) I, alpha = 1 / 2; with masks: `update`
              with lam = init and phi = 1
  factor      R' = R + (diag_load Re tr R / C + 1e-10) I = L L^H; L^-1; b = log alpha - 2 sum log L_jj.  A class whose R
              is not finite or whose R' is not positive definite is bad: L^-1 = I, b = 0
  posteriors  z = L^-1 y, q = sum |z_j|^2, phi = max(q / C, 1e-10), l = b + log a - C log phi, lam = softmax_k l.
              a_k[t] = 0: lam_k = 0; no active class: lam = 0 and no term in LL; a bin with a bad class: lam = 1 / K on
              every frame and no term in LL.  LL = sum_{t, f} max_k l + log sum_k exp(l - max)
  update      R_k = sum_t (lam_k / phi_k) y y^H / max(sum_t lam_k, 1e-10), one triangle computed and mirrored, real
              diagonal; alpha_k = max(sum_t lam_k / max(N_act, 1), 1e-10), N_act the frames with an active class
  em          init; I times factor, posteriors, update; the masks are the lam of the last posteriors.  order 'purity'
              (K = 2): per bin, class 0 becomes the class with the larger ||R||_F^2 / (Re tr R)^2; a tie keeps the order

`dtype=np.float32` rounds where the kernels round: R to complex64 and log alpha to float32, L^-1 once to complex64 and b
once to float32 after a float64 factorisation, the E-step in float32 (products and sums of z, q, l and the softmax), the
weighted sums of `update` as float32 chains in frame order per part of P frames, the parts added in float64 and rounded
once.  4 x the float32 mode's error against the float64 result is the tolerance of the device kernels:
`python tests/cgmm_ref.py` prints those errors for the cases of the GPU test.
"""
import numpy as np

P = 32                 # frames per part of the covariance pass (pykaldi2_amd.beamform.FRAMES_PER_PART)
SNAPSHOTS = (1, 3, 10)

# name -> (C, F, N, K, kind).  C in {1, 2, 3, 7, 8}; every F is 2^k + 1, so the last tile of 64 bins has one live lane; N in
# {1, P - 1, P, P + 1, 3 P + 2, 200}; K = 2 from the default start, K in {3, 4} guided: with initial masks and an
# activity, frames that are silent on every channel (with and without an active class) and whole bins of zeros.
CASES = {
    "c1_f17_n1": (1, 17, 1, 2, "plain"),
    "c2_f33_n31": (2, 33, P - 1, 2, "plain"),
    "c3_f257_n32": (3, 257, P, 2, "plain"),
    "c7_f33_n33": (7, 33, P + 1, 2, "plain"),
    "c8_f257_n98": (8, 257, 3 * P + 2, 2, "plain"),
    "c7_f257_n200": (7, 257, 200, 2, "plain"),
    "c1_f33_n98": (1, 33, 3 * P + 2, 2, "plain"),
    "c3_f33_n200_k3": (3, 33, 200, 3, "guided"),
    "c8_f17_n98_k4": (8, 17, 3 * P + 2, 4, "guided"),
    "c2_f17_n33_k3": (2, 17, P + 1, 3, "guided"),
}
RAGGED = ["r0", "r1", "r2", "r3"]      # four utterances of one minibatch: C = 3, F = 33, K = 2
RAGGED_FRAMES = [P + 1, 40, 3 * P + 2, P]


def _shape(name):
    if name in RAGGED:
        i = RAGGED.index(name)
        return 3, 33, RAGGED_FRAMES[i], 2, "plain", 900 + i
    C, F, N, K, kind = CASES[name]
    return C, F, N, K, kind, 100 + sorted(CASES).index(name)


def case_inputs(name):
    """(Y (C, N, F) complex64, init (K, N, F) float32 or None, activity (K, N) float32 or None).  K - 1 directional sources
    (rank one per bin, sparse in time and frequency) in white sensor noise 10 dB below them.  'guided': source k is active
    on its own stretch of frames (overlapping its neighbour's), the noise class everywhere; the initial masks follow the
    activity with a seeded jitter; every seventh frame is silent on every channel, every 14th of them without an active
    class; bins 3 and F - 1 are zero throughout."""
    C, F, N, K, kind, seed = _shape(name)
    r = np.random.RandomState(seed)

    def cplx(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2)
    Y = np.sqrt(0.1) * cplx(C, N, F)
    act = np.ones((K, N))
    for k in range(K - 1):
        d = r.uniform(0.7, 1.3, (C, F)) * np.exp(1j * r.uniform(0, 2 * np.pi, (C, F)))
        on = np.ones(N, bool)
        if kind == "guided":
            lo, hi = int(N * k / K), int(N * (k + 2) / K)
            on = (np.arange(N) >= lo) & (np.arange(N) < hi)
            act[k] = on
        s = cplx(N, F) * (r.uniform(0, 1, (N, F)) < 0.4) * on[:, None]
        Y = Y + d[:, None, :] * s[None]
    init = None
    if kind == "guided":
        silent = np.arange(N) % 7 == 5
        Y[:, silent, :] = 0
        act[:, np.arange(N) % 14 == 5] = 0
        Y[:, :, 3] = 0
        Y[:, :, F - 1] = 0
        init = act[:, :, None] * r.uniform(0.2, 1.0, (K, N, F))
        init = (init / np.maximum(init.sum(axis=0, keepdims=True), 1e-10)).astype(np.float32)
        act = act.astype(np.float32)
    return Y.astype(np.complex64), init, (act if kind == "guided" else None)


def _cdt(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def n_active(act, N):
    return N if act is None else int((np.asarray(act) > 0).any(axis=0).sum())


def update(Y, lam, phi=None, act=None, dtype=np.float64):
    """(R (K, F, C, C), log_alpha (K, F)) in the precision of dtype"""
    cdt = _cdt(dtype)
    Y = np.asarray(Y).astype(cdt)
    C, N, F = Y.shape
    lam = np.asarray(lam).astype(dtype)
    K = lam.shape[0]
    w = lam if phi is None else (lam / np.asarray(phi).astype(dtype)).astype(dtype)
    R = np.zeros((K, F, C, C), cdt)
    sr = np.zeros((K, F, C, C), np.complex128)
    sm = np.zeros((K, F), np.float64)
    for t0 in range(0, N, P if dtype == np.float32 else N):
        t1 = min(N, t0 + (P if dtype == np.float32 else N))
        if dtype == np.float32:
            acc, ms = np.zeros((K, F, C, C), cdt), np.zeros((K, F), dtype)
            for t in range(t0, t1):                     # frame after frame, in float32
                yy = (Y[:, None, t, :] * np.conj(Y[None, :, t, :])).astype(cdt)            # (C, C, F)
                acc = (acc + w[:, t, :, None, None] * yy.transpose(2, 0, 1)[None]).astype(cdt)
                ms = (ms + lam[:, t]).astype(dtype)
        else:
            acc = np.einsum("ktf,itf,jtf->kfij", w[:, t0:t1], Y[:, t0:t1], np.conj(Y[:, t0:t1]))
            ms = lam[:, t0:t1].sum(axis=1)
        sr += acc
        sm += ms
    den = np.maximum(sm, 1e-10)
    for i in range(C):
        for j in range(i + 1):
            v = (sr[:, :, i, j] / den).astype(cdt)
            if i == j:
                R[:, :, i, i] = v.real
            else:
                R[:, :, i, j], R[:, :, j, i] = v, np.conj(v)
    la = np.log(np.maximum(sm / max(n_active(act, N), 1), 1e-10)).astype(dtype)
    return R, la


def init_state(Y, init=None, act=None, dtype=np.float64):
    C, N, F = np.asarray(Y).shape
    if init is not None:
        return update(Y, init, None, act, dtype)
    R, la = update(Y, np.ones((2, N, F)), None, None, dtype)
    tr = np.real(np.trace(R[0].astype(np.complex128), axis1=-2, axis2=-1)) / C
    R[1] = (tr[:, None, None] * np.eye(C)).astype(R.dtype)
    la[:] = np.log(0.5)
    return R, la


def factor(R, la, diag_load=1e-3, dtype=np.float64):
    """(L^-1 (K, F, C, C) lower triangular, b (K, F), bad (K, F) bool); float64 arithmetic, rounded once in float32 mode"""
    R = np.asarray(R).astype(np.complex128)
    K, F, C, _ = R.shape
    tr = np.real(np.trace(R, axis1=-2, axis2=-1))
    Rl = R + (diag_load * tr / C + 1e-10)[..., None, None] * np.eye(C)
    Li = np.tile(np.eye(C, dtype=np.complex128), (K, F, 1, 1))
    b = np.zeros((K, F))
    bad = np.zeros((K, F), bool)
    for k in range(K):
        for f in range(F):
            ok = np.isfinite(R[k, f]).all()
            if ok:
                try:
                    L = np.linalg.cholesky(Rl[k, f])
                    X = np.linalg.inv(L)
                    ld = np.log(np.real(np.diag(L))).sum()
                    ok = np.isfinite(X).all() and np.isfinite(ld)
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                Li[k, f] = np.tril(X)
                b[k, f] = np.float64(la[k, f]) - 2 * ld
            bad[k, f] = not ok
    if dtype == np.float32:
        Li, b = Li.astype(np.complex64), b.astype(np.float32)
    return Li, b, bad


def posteriors(Y, Li, b, bad, act=None, dtype=np.float64):
    """(lam (K, N, F), phi (K, N, F), LL float64)"""
    cdt = _cdt(dtype)
    Y = np.asarray(Y).astype(cdt)
    C, N, F = Y.shape
    K = Li.shape[0]
    Li, b = Li.astype(cdt), b.astype(dtype)
    q = np.zeros((K, N, F), dtype)
    for i in range(C):
        z = np.zeros((K, N, F), cdt)
        for j in range(i + 1):                          # ascending column order
            z = (z + Li[:, None, :, i, j] * Y[None, j]).astype(cdt)
        q = (q + (z.real * z.real).astype(dtype)).astype(dtype)
        q = (q + (z.imag * z.imag).astype(dtype)).astype(dtype)
    phi = np.maximum((q / dtype(C)).astype(dtype), dtype(1e-10))
    with np.errstate(divide="ignore"):
        loga = np.zeros((K, N), dtype) if act is None else np.log(np.asarray(act).astype(dtype))
    ell = ((b[:, None, :] + loga[:, :, None]).astype(dtype) - (dtype(C) * np.log(phi)).astype(dtype)).astype(dtype)
    mx = ell.max(axis=0)
    live = mx > -np.inf
    with np.errstate(invalid="ignore"):
        e = np.where(live[None], np.exp((ell - np.where(live, mx, 0)[None]).astype(dtype)), 0).astype(dtype)
    s = e.sum(axis=0, dtype=dtype)
    lam = np.where(live[None], e / np.where(live, s, 1)[None], 0).astype(dtype)
    term = np.where(live, mx + np.log(np.where(live, s, 1)).astype(dtype), 0).astype(dtype)
    fail = bad.any(axis=0)
    lam[:, :, fail] = dtype(1.0) / dtype(K)
    term[:, fail] = 0
    return lam, phi, float(term.astype(np.float64).sum())


def purity(R):
    R = np.asarray(R).astype(np.complex128)
    tr = np.real(np.trace(R, axis1=-2, axis2=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(R) ** 2).sum(axis=(-2, -1)) / tr ** 2


def reorder(lam, R, la):
    """the purity order for K = 2: (lam, R, la, swapped (F,) bool)"""
    p = purity(R)
    swap = p[1] > p[0]
    lam, R, la = lam.copy(), R.copy(), la.copy()
    lam[:, :, swap] = lam[::-1][:, :, swap]
    R[:, swap] = R[::-1][:, swap]
    la[:, swap] = la[::-1][:, swap]
    return lam, R, la, swap


def em(Y, iterations=10, init=None, act=None, diag_load=1e-3, order=None, dtype=np.float64, snapshots=()):
    """dict(masks, R, la, ll (iterations,), nonfinite, swapped, and snap: iteration -> (masks, R, la) in the order asked
    for, for every iteration of `snapshots`)"""
    order = order or ("purity" if init is None else "keep")
    R, la = init_state(Y, init, act, dtype)
    K = R.shape[0]
    if order == "purity" and K != 2:
        raise ValueError("the purity order is defined for two classes")
    ll, nonfinite, snap = [], False, {}
    for it in range(1, iterations + 1):
        Li, b, bad = factor(R, la, diag_load, dtype)
        nonfinite = nonfinite or bool(bad.any())
        lam, _phi, l = posteriors(Y, Li, b, bad, act, dtype)
        ll.append(l)
        R, la = update(Y, lam, _phi, act, dtype)
        if it in snapshots or it == iterations:
            snap[it] = reorder(lam, R, la) if order == "purity" else (lam, R, la, np.zeros(R.shape[1], bool))
    lam, R, la, swapped = snap[iterations]
    return dict(masks=lam, R=R, la=la, ll=np.array(ll), nonfinite=nonfinite, swapped=swapped, snap=snap)


def scene(C, seed, N=300, F=9, snr_db=10.0):
    """A rank-one source in white noise at `snr_db`, sparse in time and frequency: (Y (C, N, F) complex128, ideal (N, F)
    bool: the points where the source is on)."""
    r = np.random.RandomState(seed)

    def cplx(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2)
    d = np.exp(1j * r.uniform(0, 2 * np.pi, (C, F)))
    on = r.uniform(0, 1, (N, F)) < 0.35
    s = cplx(N, F) * on
    return d[:, None, :] * s[None] + 10 ** (-snr_db / 20) * cplx(C, N, F), on


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def float32_errors(name):
    """The float32 mode against float64 on a case: dict of the largest errors of the stage functions (given the float64
    inputs) and of the whole EM at every snapshot (masks absolute, the rest relative to max |want|)."""
    Y, init, act = case_inputs(name)
    w = em(Y, 10, init, act, order="keep", snapshots=SNAPSHOTS)
    g = em(Y, 10, init, act, order="keep", dtype=np.float32, snapshots=SNAPSHOTS)
    out = {"masks": 0.0, "cov": 0.0, "la": 0.0, "ll": rel(g["ll"], w["ll"])}
    for it in SNAPSHOTS:
        out["masks"] = max(out["masks"], float(np.abs(g["snap"][it][0] - w["snap"][it][0]).max()))
        out["cov"] = max(out["cov"], rel(g["snap"][it][1], w["snap"][it][1]))
        out["la"] = max(out["la"], rel(g["snap"][it][2], w["snap"][it][2]))
    s = stages(name)
    R032, la032 = init_state(Y, init, act, np.float32)
    out["init"], out["init_log_alpha"] = rel(R032, s["R0"]), rel(la032, s["la0"])
    Li32, b32, _ = factor(s["R32"], s["la32"], dtype=np.float32)
    out["linv"], out["bias"] = rel(Li32, s["Li"]), rel(b32, s["b"])
    lam32, phi32, l32 = posteriors(Y, s["Li32"], s["b32"], s["bad"], act, np.float32)
    out["lam"], out["phi"] = float(np.abs(lam32 - s["lam"]).max()), rel(phi32, s["phi"])
    out["ll1"] = abs(l32 - s["ll"]) / abs(s["ll"])
    Ru32, lau32 = update(Y, s["lam32"], s["phi32"], act, np.float32)
    out["update"], out["log_alpha"] = rel(Ru32, s["Ru"]), rel(lau32, s["lau"])
    return out


def stages(name):
    """What the stage tests compare with, every stage in float64 on the float32 values the stage before it hands over:
    the start state (R0, la0) and its rounding (R32, la32); their factor (Li, b, bad) and its rounding (Li32, b32); the
    posteriors of that (lam, phi, ll) and their roundings (lam32, phi32); the update of those (Ru, lau)."""
    Y, init, act = case_inputs(name)
    s = dict(Y=Y, init=init, act=act)
    s["R0"], s["la0"] = init_state(Y, init, act)
    s["R32"], s["la32"] = s["R0"].astype(np.complex64), s["la0"].astype(np.float32)
    s["Li"], s["b"], s["bad"] = factor(s["R32"], s["la32"])
    s["Li32"], s["b32"] = s["Li"].astype(np.complex64), s["b"].astype(np.float32)
    s["lam"], s["phi"], s["ll"] = posteriors(Y, s["Li32"], s["b32"], s["bad"], act)
    s["lam32"], s["phi32"] = s["lam"].astype(np.float32), s["phi"].astype(np.float32)
    s["Ru"], s["lau"] = update(Y, s["lam32"], s["phi32"], act)
    return s


def pack_linv(Li):
    """(K, F, C, C) lower triangular -> the device layout (K, C (C + 1), F): the lower triangle row by row, (re, im) planes"""
    K, F, C, _ = Li.shape
    out = np.zeros((K, C * (C + 1), F), np.float32)
    p = 0
    for i in range(C):
        for j in range(i + 1):
            out[:, 2 * p], out[:, 2 * p + 1] = Li[:, :, i, j].real, Li[:, :, i, j].imag
            p += 1
    return out


def unpack_linv(planes, C):
    K, _, F = planes.shape
    Li = np.zeros((K, F, C, C), np.complex128)
    p = 0
    for i in range(C):
        for j in range(i + 1):
            Li[:, :, i, j] = planes[:, 2 * p] + 1j * planes[:, 2 * p + 1]
            p += 1
    return Li


GOLDEN_RIR = "cgmm_rir_c4.npy"      # tests/golden: float32 (4, 3200), pykaldi2_amd.rirgen.xp_rirgen for RIR_SETUP
RIR_SETUP = dict(room=(5.0, 4.0, 3.0), source=(3.6, 2.9, 1.6), centre=(2.0, 1.5, 1.2), n_mics=4, radius=0.05, t60=0.2)


def write_golden_rir(path):
    """How tests/golden/cgmm_rir_c4.npy was made (needs the GPU: pykaldi2_amd.rirgen)"""
    from pykaldi2_amd import beamform, rirgen
    s = RIR_SETUP
    mic = np.asarray(s["centre"], np.float64)[:, None] + beamform.array_geometry(s["n_mics"], s["radius"])
    rir = rirgen.xp_rirgen(np.asarray(s["room"], np.float64), np.asarray(s["source"], np.float64)[:, None], mic, t60=s["t60"])
    np.save(path, rir[0].cpu().numpy().astype(np.float32))


def rir_scene(rir, seed=7, n=16000, snr_db=5.0):
    """A directional speech-like source through the (C, k) RIRs of one room plus white sensor noise `snr_db` below its image
    at microphone 0: (wav (C, n) float32, that image (n,) float64)."""
    import mask_ref
    r = np.random.RandomState(seed)
    s = mask_ref.inputs(seed, n, 5)[0].astype(np.float64)
    img = np.stack([np.convolve(s, h.astype(np.float64))[:n] for h in rir])
    noise = r.standard_normal(img.shape) * np.sqrt(np.mean(img[0] ** 2) * 10 ** (-snr_db / 10))
    return (img + noise).astype(np.float32), img[0]


def enhance(wav, iterations=10, dtype=np.float64):
    """The restatement of MaskBeamformer(mask_estimator=CgmmMaskEstimator(...))(wav): STFT, two-class cGMM masks in the
    purity order, MVDR with both masks, inverse STFT cut to the input's length"""
    import beamform_ref
    import mask_ref
    Y = beamform_ref.spectrum(wav, mask_ref.DEFAULT, dtype)
    m = em(Y, iterations, dtype=dtype)["masks"]
    phi = beamform_ref.covariance(Y, m, False, dtype)
    w, _ = beamform_ref.mvdr_weights(phi[0], phi[1], 0)
    y, _ = mask_ref.istft(beamform_ref.apply(Y, w, dtype), dtype=dtype, **mask_ref.DEFAULT)
    return y[:wav.shape[1]]


if __name__ == "__main__":
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_RIR)
    if os.path.exists(gold):
        import beamform_ref
        wav, target = rir_scene(np.load(gold))
        print("SI-SDR gain of the restatement on the RIR scene: %.2f dB"
              % beamform_ref.scene_gain(enhance(wav), wav, target))
    worst = {}
    for name in list(CASES) + RAGGED:
        e = float32_errors(name)
        print(name, " ".join("%s %.2e" % kv for kv in sorted(e.items())))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
