"""Restatement of the mask-based MVDR beamformer -- TEST INFRASTRUCTURE ONLY (tests/ and tools/ import
it; the product path never does).  The reference project has no beamformer: this numpy float64 text is the oracle.

For one utterance with spectrum Y (C, N, F) complex (channel- and frame-major, mask_ref.stft per channel) and masks m_k
(N, F):

  covariance   Phi_k[f] = sum_t m_k[t, f] y y^H / max(sum_t m_k[t, f], 1e-10), y = Y[:, t, f]: (K, F, C, C), one triangle
               computed and mirrored, real diagonal; complement=True (one mask): the matrices of m and of 1 - m
  loading      Phi_n' = Phi_n + (diag_load Re tr(Phi_n) / C + 1e-10) I
  weights      G = Phi_n'^-1 Phi_s (numpy.linalg.solve), w = G[:, r] / tr G; w = e_r where |tr G| <= 1e-20: (F, C)
  'snr'        r = argmax_c sum_f Re(w^(c)H Phi_s w^(c)) / sum_f Re(w^(c)H Phi_n' w^(c)), ties to the lowest c
  apply        X[t, f] = sum_c conj(w[f, c]) Y[c, t, f]: (N, F)

`dtype=np.float32` runs the sums of covariance and apply in single precision (products and additions in complex64 /
float32, frame after frame); the solve is always float64, as on the device.  4 x the float32 mode's error against the
float64 result is the tolerance of the device kernels.
"""
import numpy as np

import mask_ref

CFGS = {17: dict(fft_size=32, frame_len=32, frame_shift=8, window="hann"),
        33: dict(fft_size=64, frame_len=64, frame_shift=16, window="hann"),
        257: dict(fft_size=512, frame_len=400, frame_shift=160, window="hamming")}
P = 32      # the covariance kernel's frames per workgroup (pykaldi2_amd.beamform.FRAMES_PER_PART; the host test compares)

# name -> (C, F, N, K, complement, mask kind).  C in {1, 2, 3, 8} (and the data path's 7); every F is 2^k + 1, so the last
# tile of 64 bins has one live lane; N in {1, P - 1, P, P + 1, 3 P + 2} and 200 (seven partials per bin tile); K in
# {1, 2, 4} and the complement; masks that are zero on whole bins and on whole frames.
CASES = {
    "c1_f17_n1_k1": (1, 17, 1, 1, False, "ratio"),
    "c2_f33_n31_k2": (2, 33, P - 1, 2, False, "ratio"),
    "c3_f257_n32_k4": (3, 257, P, 4, False, "ratio"),
    "c8_f17_n33_comp": (8, 17, P + 1, 1, True, "ratio"),
    "c8_f257_n98_k2": (8, 257, 3 * P + 2, 2, False, "ratio"),
    "c3_f33_n200_comp": (3, 33, 200, 1, True, "ratio"),
    "c1_f257_n33_comp": (1, 257, P + 1, 1, True, "ratio"),
    "c7_f257_n98_comp": (7, 257, 3 * P + 2, 1, True, "ratio"),
    "c2_f257_n98_zero_bins": (2, 257, 3 * P + 2, 1, True, "zero_bins"),
    "c8_f33_n98_k4_zero_frames": (8, 33, 3 * P + 2, 4, False, "zero_frames"),
}
SNR_CASES = ["c2_f33_n31_k2", "c8_f257_n98_k2", "c3_f33_n200_comp", "c7_f257_n98_comp"]      # margins: the host test
RAGGED = ["c3_b0", "c3_b1", "c3_b2", "c3_b3"]      # four utterances of one minibatch: C = 3, F = 33, K = 1 + complement
RAGGED_FRAMES = [P + 1, 1, 3 * P + 2, P]


def case_inputs(name):
    """(Y (C, N, F) complex64, masks (K, N, F) float32) of a case: a speech and a noise component with their own
    per-channel gains and phases plus a sensor-noise floor, the first mask the speech's ratio mask at channel 0, the
    second the noise's, further ones uniform draws."""
    if name in RAGGED:
        i = RAGGED.index(name)
        C, F, N, K, kind, seed = 3, 33, RAGGED_FRAMES[i], 1, "ratio", 900 + i
    else:
        C, F, N, K, _, kind = CASES[name]
        seed = 100 + sorted(CASES).index(name)
    r = np.random.RandomState(seed)

    def cplx(*shape):
        return r.standard_normal(shape) + 1j * r.standard_normal(shape)
    act_s, act_n = r.uniform(0, 1, (N, F)) ** 4, r.uniform(0, 1, (N, F)) ** 2      # sparse speech, denser noise
    # The output SNR of an MVDR filter does not depend on its reference channel bin by bin; summed over the bins it favours
    # the channel that is loud where the bins are clean.  The noise grows with f and channel c weighs the bins by
    # exp(a_c cos(pi f / F)), a_c rising with c, so the channels' SNRs are well apart (asserted in the host test).
    tilt = np.cos(np.pi * np.arange(F) / F)[None, :]
    S, V = cplx(N, F) * act_s, (0.3 + 1.5 * np.arange(F) / F)[None, :] * cplx(N, F) * act_n
    ds = np.exp(0.5 * (np.arange(C)[:, None] - (C - 1) / 2) * tilt) * np.exp(1j * r.uniform(0, 2 * np.pi, (C, F)))
    dn = (1.5 - np.arange(C)[:, None] / C) * np.exp(1j * r.uniform(0, 2 * np.pi, (C, F)))
    Y = ds[:, None, :] * S[None] + dn[:, None, :] * V[None] + 0.05 * cplx(C, N, F)
    ps, pn = np.abs(ds[0] * S) ** 2, np.abs(dn[0] * V) ** 2 + 0.005
    masks = [ps / (ps + pn), pn / (ps + pn)] + [r.uniform(0, 1, (N, F)) for _ in range(2)]
    masks = np.stack(masks[:K]).astype(np.float32)
    if kind == "zero_bins":
        masks[:, :, ::5] = 0
        masks[:, :, F - 1] = 0
    elif kind == "zero_frames":
        masks[:, ::3, :] = 0
    return Y.astype(np.complex64), masks


def covariance(Y, masks, complement=False, dtype=np.float64):
    """(K, F, C, C) complex (K = 2 with complement) in the precision of `dtype`"""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    Y = np.asarray(Y).astype(cdt)
    m = np.asarray(masks).astype(dtype)
    m = m[None] if m.ndim == 2 else m
    if complement:
        if m.shape[0] != 1:
            raise ValueError("complement takes exactly one mask")
        m = np.concatenate([m, dtype(1) - m])
    C, N, F = Y.shape
    out = np.zeros((m.shape[0], F, C, C), cdt)
    for k in range(m.shape[0]):
        den = np.maximum(m[k].sum(axis=0, dtype=dtype), dtype(1e-10))
        for i in range(C):
            for j in range(i + 1):
                acc = np.zeros(F, cdt)
                prod = (Y[i] * np.conj(Y[j])).astype(cdt)
                for t in range(N):                      # frame after frame, in the precision of dtype
                    acc = (acc + m[k, t] * prod[t]).astype(cdt)
                v = (acc / den).astype(cdt)
                if i == j:
                    out[k, :, i, i] = v.real
                else:
                    out[k, :, i, j], out[k, :, j, i] = v, np.conj(v)
    return out


def load(phi_n, diag_load=1e-3):
    phi_n = np.asarray(phi_n).astype(np.complex128)
    C = phi_n.shape[-1]
    tr = np.real(np.trace(phi_n, axis1=-2, axis2=-1))
    return phi_n + (diag_load * tr / C + 1e-10)[:, None, None] * np.eye(C)


def _weights_all(phi_s, phi_n, diag_load):
    """candidates (C, F, C): w^(r)[f, :] for every r; and Phi_n'"""
    phi_s = np.asarray(phi_s).astype(np.complex128)
    pn = load(phi_n, diag_load)
    F, C = phi_s.shape[0], phi_s.shape[1]
    G = np.linalg.solve(pn, phi_s)
    tr = np.trace(G, axis1=-2, axis2=-1)
    cand = np.zeros((C, F, C), np.complex128)
    for r in range(C):
        for f in range(F):
            cand[r, f] = G[f, :, r] / tr[f] if abs(tr[f]) > 1e-20 else np.eye(C)[r]
    return cand, pn


def snr_per_channel(phi_s, phi_n, diag_load=1e-3):
    cand, pn = _weights_all(phi_s, phi_n, diag_load)
    ps = np.asarray(phi_s).astype(np.complex128)
    num = np.einsum("rfi,fij,rfj->r", cand.conj(), ps, cand).real
    den = np.einsum("rfi,fij,rfj->r", cand.conj(), pn, cand).real
    return num / den


def mvdr_weights(phi_s, phi_n, ref=0, diag_load=1e-3):
    """(w (F, C) complex128, r); float64 whatever the precision of the covariances"""
    cand, _ = _weights_all(phi_s, phi_n, diag_load)
    if ref == "snr":
        ref = int(np.argmax(snr_per_channel(phi_s, phi_n, diag_load)))        # argmax: the first maximum
    return cand[ref], ref


def tie_covariances(F=17, C=3):
    """Phi_s = 2 I and Phi_n = I at every bin: every channel's weights are e_c / C and every SNR the same number"""
    eye = np.tile(np.eye(C, dtype=np.complex64), (F, 1, 1))
    return 2 * eye, eye.copy()


def apply(Y, w, dtype=np.float64):
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    Y, w = np.asarray(Y).astype(cdt), np.asarray(w).astype(cdt)
    X = np.zeros(Y.shape[1:], cdt)
    for c in range(Y.shape[0]):
        X = (X + np.conj(w[:, c])[None, :] * Y[c]).astype(cdt)
    return X


def spectrum(wav, cfg, dtype=np.float64):
    return np.stack([mask_ref.stft(x, dtype=dtype, **cfg) for x in wav])


def beamform(wav, speech_mask, noise_mask=None, cfg=mask_ref.DEFAULT, ref=0, diag_load=1e-3, dtype=np.float64):
    """wav (C, n) -> (enhanced (n,), window sum (n,), w, r): end to end with mask_ref.stft / istft"""
    Y = spectrum(wav, cfg, dtype)
    if noise_mask is None:
        phi = covariance(Y, speech_mask, True, dtype)
    else:
        phi = covariance(Y, np.stack([speech_mask, noise_mask]), False, dtype)
    w, r = mvdr_weights(phi[0], phi[1], ref, diag_load)
    y, ws = mask_ref.istft(apply(Y, w, dtype), dtype=dtype, **cfg)
    n = wav.shape[1]
    return y[:n], ws[:n], w, r


def e2e_inputs(F, C, n, seed):
    """(wav (C, n) float32, speech mask (N, F) float32): two mask_ref.inputs signals through per-channel integer delays and
    gains, the mask the first one's ratio mask at channel 0"""
    cfg = CFGS[F]
    r = np.random.RandomState(seed)
    s, v = mask_ref.inputs(seed, n, 5)[0].astype(np.float64), mask_ref.inputs(seed + 50, n, 5)[0].astype(np.float64)
    img_s = np.stack([r.uniform(0.7, 1.0) * np.roll(s, int(d)) for d in r.randint(0, 4, C)])
    img_v = np.stack([r.uniform(0.7, 1.0) * np.roll(v, int(d)) for d in r.randint(0, 4, C)])
    wav = (img_s + img_v + 1e-3 * r.standard_normal((C, n))).astype(np.float32)
    ps = np.abs(mask_ref.stft(img_s[0], **cfg)) ** 2
    pv = np.abs(mask_ref.stft(img_v[0], **cfg)) ** 2 + 1e-8
    return wav, (ps / (ps + pv)).astype(np.float32)


E2E_CASES = {"f257_c4": (257, 4, 6000, 21), "f33_c2": (33, 2, 1000, 22)}


def si_sdr(est, ref):
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    a = np.dot(est, ref) / np.dot(ref, ref)
    return 10 * np.log10(np.sum((a * ref) ** 2) / np.sum((est - a * ref) ** 2))


def scene(seed=7, C=4, n=16000):
    """A seeded anechoic scene: a target and an interferer of equal level, each with per-microphone integer delays and
    gains, and weak sensor noise.  Returns (wav (C, n) float32, the target's image at microphone 0 (n,), ideal ratio mask
    (N, F) float32 from the known components at microphone 0)."""
    r = np.random.RandomState(seed)
    s = mask_ref.inputs(seed, n, 5)[0].astype(np.float64)
    v = mask_ref.inputs(seed + 1, n, 5)[0].astype(np.float64)
    v *= np.sqrt(np.mean(s ** 2) / np.mean(v ** 2))
    ds, dv = [0, 2, 4, 6][:C], [5, 3, 1, 0][:C]
    gs, gv = r.uniform(0.8, 1.0, C), r.uniform(0.8, 1.0, C)
    img_s = np.stack([g * np.roll(s, d) for g, d in zip(gs, ds)])
    img_v = np.stack([g * np.roll(v, d) for g, d in zip(gv, dv)])
    noise = 1e-3 * r.standard_normal((C, n))
    ps = np.abs(mask_ref.stft(img_s[0])) ** 2
    pv = np.abs(mask_ref.stft(img_v[0] + noise[0])) ** 2
    return (img_s + img_v + noise).astype(np.float32), img_s[0], (ps / (ps + pv + 1e-12)).astype(np.float32)


def scene_gain(enhanced, wav, target):
    """SI-SDR of the output against the target's image at the reference microphone minus the reference channel's own"""
    return si_sdr(enhanced, target) - si_sdr(wav[0], target)
