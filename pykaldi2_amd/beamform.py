"""Mask-based MVDR beamforming on the device (csrc/beamform.hip): from a (C, T) array signal and a
time-frequency mask to the one waveform the filterbank and the acoustic models take.

  spatial_covariance(spec, masks, complement)   Phi_k[f] = sum_t m_k y y^H / max(sum_t m_k, 1e-10): complex64 (K, F, C, C)
  mvdr_weights(phi_s, phi_n, ref, diag_load)     Souden's MVDR, w[f] = G[:, r] / tr G with G = Phi_n'^-1 Phi_s: (w (F, C), r)
  apply_weights(spec, w)                         X[t, f] = sum_c conj(w[f, c]) Y[c, t, f]: complex64 (N, F)
  MaskBeamformer(analyzer, ref, diag_load)       wav (C, n), speech mask (N, F) -> enhanced float32 (n,)

Spectra are complex64 (C, N, F), channel- and frame-major, as SpectrumAnalyzer.analyze returns them for a (C, n) signal;
masks are float32 (N, F) like MaskEstimator's; 1 <= C <= 8, 1 <= K <= 4.  Every function also takes lists, one entry per
utterance of a ragged minibatch (common C, F, K), and then makes one launch per stage for the list.  `ref` is a channel or
'snr' (the channel whose weights give the largest output SNR, chosen on the device); the choice and the non-finite flag stay
in device tensors.  Nothing is read back to the host.

  beamform_config(config) / require_beamform_config(config, prog)     the data_config key `beamform` (needs no GPU)
  array_geometry(n_mics, radius)                                      the (3, C) microphone offsets of that key
"""
import math
import sys

import numpy as np
import torch

from . import _lib
from ._array import _as_list, _check_specs, _diag_load_arg, _frames, _table, analyze_channels

MAX_CHANNELS, MAX_MASKS = _lib.BF_MAX_CHANNELS, _lib.BF_MAX_MASKS
FRAMES_PER_PART = _lib.BF_FRAMES_PER_PART      # frames per workgroup of the covariance pass
CONFIG_DEFAULTS = dict(n_mics=7, radius=0.0425, ref=0, diag_load=0.001)
MASK_KEYS = ("mask", "cgmm_iterations")        # optional: present in beamform_config's result only when the mapping has one

last_nonfinite = None      # CUDA int32 (B,) of the last mvdr_weights call: 1 where an utterance had a non-finite bin


def _workspace(frames, B, Cn, F, K, complement, dev):
    fr = _frames(frames) if frames is not None else None
    nbytes = _lib.lib().pk2_bf_workspace_bytes(fr, B, Cn, F, K, int(complement))
    if nbytes == 0:
        raise ValueError("beamform: no workspace for B %d, C %d, F %d, K %d" % (B, Cn, F, K))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def spatial_covariance(spec, masks, complement=False):
    """spec: complex64 (C, N, F); masks: float32 (N, F), (K, N, F) or a list of K (N, F) tensors.  Returns complex64
    (K, F, C, C), exactly Hermitian; complement=True (one mask m): (2, F, C, C), for m and for 1 - m, from one pass.
    Lists of both (one entry per utterance): one launch, and a list of results."""
    _lib.require_gpu()
    specs, many, Cn, F, dev = _check_specs(spec, "spatial_covariance", MAX_CHANNELS)
    mlist = list(masks) if many else [masks]
    if len(mlist) != len(specs):
        raise ValueError("spatial_covariance: %d spectra, %d entries of masks" % (len(specs), len(mlist)))
    rows, K = [], None
    for i, (s, m) in enumerate(zip(specs, mlist)):
        if isinstance(m, torch.Tensor):
            m = [m] if m.dim() == 2 else list(m.unbind(0)) if m.dim() == 3 else [m]
        m = list(m)
        K = len(m) if K is None else K
        if len(m) != K or not 1 <= K <= MAX_MASKS:
            raise ValueError("spatial_covariance: utterance %d has %d masks, expected %d (1 to %d)" % (i, len(m), K, MAX_MASKS))
        for k, mk in enumerate(m):
            if not (isinstance(mk, torch.Tensor) and mk.is_cuda and mk.dtype == torch.float32 and mk.device == dev
                    and mk.is_contiguous()):
                raise ValueError("spatial_covariance: utterance %d, mask %d: expected a contiguous CUDA float32 tensor on %s"
                                 % (i, k, dev))
            if tuple(mk.shape) != (s.shape[1], F):
                raise ValueError("spatial_covariance: utterance %d, mask %d has shape %r, the spectrum (N, F) = (%d, %d)"
                                 % (i, k, tuple(mk.shape), s.shape[1], F))
        rows.extend(m)
    if complement and K != 1:
        raise ValueError("spatial_covariance: complement=True takes exactly one mask, got %d" % K)
    B, KA = len(specs), 2 if complement else K
    frames = [int(s.shape[1]) for s in specs]
    phi = torch.empty(B, KA, F, Cn, Cn, dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, B, Cn, F, K, complement, dev)
        _lib.check(_lib.lib().pk2_bf_cov(_table(specs), _table(rows), _frames(frames), B, Cn, F, K, int(bool(complement)),
                                         _lib.ptr(work), nbytes, _lib.ptr(phi), _lib.stream_ptr(dev)))
    return list(phi.unbind(0)) if many else phi[0]


def _ref_arg(ref, Cn, who):
    if isinstance(ref, str):
        if ref != 'snr':
            raise ValueError("%s: ref must be a channel index or 'snr', got %r" % (who, ref))
        return _lib.BF_REF_SNR
    if isinstance(ref, bool) or not isinstance(ref, (int, np.integer)):
        raise ValueError("%s: ref must be a channel index or 'snr', got %r" % (who, ref))
    if Cn is not None and not 0 <= int(ref) < Cn:
        raise ValueError("%s: ref %d outside the %d channels" % (who, int(ref), Cn))
    if int(ref) < 0:
        raise ValueError("%s: ref %d is negative" % (who, int(ref)))
    return int(ref)


def mvdr_weights(phi_s, phi_n, ref=0, diag_load=1e-3):
    """phi_s, phi_n: complex64 (F, C, C) (the two matrices of spatial_covariance).  Returns (w complex64 (F, C), ref_index
    CUDA int32 (1,)); for lists, (list of w, ref_index (B,)).  The solve runs in float64 on the device.  A bin with an empty
    speech mask, or with non-finite input, passes the reference channel through (w = e_r); the module's `last_nonfinite`
    (CUDA int32, one entry per utterance) tells the latter apart and is not read back here."""
    global last_nonfinite
    _lib.require_gpu()
    ps, many = _as_list(phi_s, "mvdr_weights")
    pn = list(phi_n) if many else [phi_n]
    if len(ps) != len(pn):
        raise ValueError("mvdr_weights: %d speech covariances, %d noise covariances" % (len(ps), len(pn)))
    for i, (a, b) in enumerate(zip(ps, pn)):
        for what, p in (("phi_s", a), ("phi_n", b)):
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.complex64 and p.dim() == 3
                    and p.is_contiguous() and p.shape[1] == p.shape[2] and p.numel() > 0):
                raise ValueError("mvdr_weights: utterance %d: %s must be a contiguous CUDA complex64 (F, C, C) tensor" % (i, what))
        if a.shape != ps[0].shape or b.shape != ps[0].shape or a.device != ps[0].device or b.device != ps[0].device:
            raise ValueError("mvdr_weights: utterance %d: phi_s %r and phi_n %r must both be %r on %s"
                             % (i, tuple(a.shape), tuple(b.shape), tuple(ps[0].shape), ps[0].device))
    F, Cn, dev = ps[0].shape[0], ps[0].shape[1], ps[0].device
    if Cn > MAX_CHANNELS:
        raise ValueError("mvdr_weights: %d channels, at most %d" % (Cn, MAX_CHANNELS))
    r = _ref_arg(ref, Cn, "mvdr_weights")
    diag_load = _diag_load_arg(diag_load, "mvdr_weights")
    B = len(ps)
    w = torch.empty(B, F, Cn, dtype=torch.complex64, device=dev)
    ref_index = torch.empty(B, dtype=torch.int32, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(None, B, Cn, F, 1, False, dev)
        _lib.check(_lib.lib().pk2_bf_mvdr_weights(_table(ps), _table(pn), B, Cn, F, r, diag_load, _lib.ptr(work), nbytes,
                                                  _lib.ptr(w), _lib.ptr(ref_index), _lib.ptr(flag), _lib.stream_ptr(dev)))
    last_nonfinite = flag
    return (list(w.unbind(0)), ref_index) if many else (w[0], ref_index)


def apply_weights(spec, w):
    """spec: complex64 (C, N, F); w: complex64 (F, C).  Returns complex64 (N, F); lists -> one launch, a list."""
    _lib.require_gpu()
    specs, many, Cn, F, dev = _check_specs(spec, "apply_weights", MAX_CHANNELS)
    ws = list(w) if many else [w]
    if len(ws) != len(specs):
        raise ValueError("apply_weights: %d spectra, %d weight matrices" % (len(specs), len(ws)))
    for i, wi in enumerate(ws):
        if not (isinstance(wi, torch.Tensor) and wi.is_cuda and wi.dtype == torch.complex64 and wi.is_contiguous()
                and wi.device == dev):
            raise ValueError("apply_weights: utterance %d: w must be a contiguous CUDA complex64 tensor on %s" % (i, dev))
        if tuple(wi.shape) != (F, Cn):
            raise ValueError("apply_weights: utterance %d: w has shape %r, the spectrum (F, C) = (%d, %d)"
                             % (i, tuple(wi.shape), F, Cn))
    frames = [int(s.shape[1]) for s in specs]
    outs = [torch.empty(n, F, dtype=torch.complex64, device=dev) for n in frames]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_bf_apply(_table(specs), _table(ws), _frames(frames), len(specs), Cn, F, _table(outs),
                                           _lib.stream_ptr(dev)))
    return outs if many else outs[0]


class MaskBeamformer:
    """analyzer: a simulation.SpectrumAnalyzer (its FFT size, frame and window; the analysis here never dithers, whatever
    the analyzer's do_dither).  __call__(wav (C, n), speech_mask (N, F), noise_mask=None) -> float32 (n,): STFT, covariances
    of the speech mask and of the noise mask (None: 1 - speech_mask, from the same pass), MVDR weights, the weighted sum and
    the inverse STFT cut to n.  `batch` does it for a ragged list with one launch per beamforming stage (the STFT entries
    take one length per call).  `last_weights` ((F, C), or the list), `last_ref` and `last_nonfinite` (CUDA int32, one entry
    per utterance) keep the last call's and are not read back.  mask_estimator (cgmm.CgmmMaskEstimator, or any object
    whose masks(list of spectra) returns one (speech mask, noise mask) per spectrum): with it speech_mask may be None and
    both masks are estimated from the array spectrum; without it None is a ValueError.  Calls that pass masks never use it."""

    def __init__(self, analyzer, ref=0, diag_load=1e-3, mask_estimator=None):
        self.analyzer = analyzer
        _ref_arg(ref, None, "MaskBeamformer")
        self.ref, self.diag_load = ref, _diag_load_arg(diag_load, "MaskBeamformer")
        if mask_estimator is not None and not callable(getattr(mask_estimator, "masks", None)):
            raise ValueError("MaskBeamformer: mask_estimator must have masks(list of spectra) -> list of (speech mask, noise "
                             "mask), like cgmm.CgmmMaskEstimator")
        self.mask_estimator = mask_estimator
        self.last_weights = self.last_ref = self.last_nonfinite = None

    def analyze(self, wav):
        """(C, n) CUDA float32 -> complex64 (C, N, F), without dither"""
        return analyze_channels(self.analyzer, wav, "MaskBeamformer", MAX_CHANNELS)

    def batch(self, wavs, speech_masks=None, noise_masks=None):
        wavs = list(wavs)
        if speech_masks is None:
            if self.mask_estimator is None:
                raise ValueError("MaskBeamformer: no speech mask and no mask_estimator")
            if noise_masks is not None:
                raise ValueError("MaskBeamformer: a noise mask without a speech mask")
            specs = [self.analyze(x) for x in wavs]
            pairs = self.mask_estimator.masks(specs)
            speech_masks, noise_masks = [p[0] for p in pairs], [p[1] for p in pairs]
        else:
            speech_masks = list(speech_masks)
            if len(speech_masks) != len(wavs) or (noise_masks is not None and len(noise_masks) != len(wavs)):
                raise ValueError("MaskBeamformer: one speech mask (and noise mask) per waveform")
            specs = [self.analyze(x) for x in wavs]
        if noise_masks is None:
            phi = spatial_covariance(specs, speech_masks, complement=True)
        else:
            phi = spatial_covariance(specs, [[s, n] for s, n in zip(speech_masks, noise_masks)])
        w, self.last_ref = mvdr_weights([p[0] for p in phi], [p[1] for p in phi], self.ref, self.diag_load)
        self.last_weights, self.last_nonfinite = w, last_nonfinite
        enhanced = apply_weights(specs, w)
        return [self.analyzer.synthesize(X)[:x.shape[1]] for X, x in zip(enhanced, wavs)]

    def __call__(self, wav, speech_mask=None, noise_mask=None):
        out = self.batch([wav], None if speech_mask is None else [speech_mask], None if noise_mask is None else [noise_mask])[0]
        self.last_weights = self.last_weights[0]
        return out


def array_geometry(n_mics=7, radius=0.0425):
    """The (3, C) offsets of a uniform circular array in the horizontal plane from its centre (rirgen.sample_array's
    `mic_positions`).  n_mics = 7 is the usual 7-channel device: channel 0 at the centre and six on the circle; any other
    count puts all microphones on the circle, channel c at angle 2 pi c / n_mics."""
    n = int(n_mics)
    pos = np.zeros((3, n))
    ring = np.arange(n - 1) if n == 7 else np.arange(n)
    ang = 2.0 * np.pi * ring / len(ring)
    pos[0, n - len(ring):] = float(radius) * np.cos(ang)
    pos[1, n - len(ring):] = float(radius) * np.sin(ang)
    return pos


def beamform_config(config):
    """data_config `beamform`: true (the defaults n_mics 7, radius 0.0425 m, ref 0, diag_load 0.001) or a mapping over them;
    None when the key is absent or false.  The mapping may also hold `mask: ideal | cgmm` (default ideal: the simulated
    source's ideal mask; cgmm: masks estimated from the array spectrum, pykaldi2_amd.cgmm) and `cgmm_iterations` (10). Raises ValueError for a bad value and for a configuration that cannot honour the
    key: it needs `online_rir: true`, `use_reverb: true` and `simulation_prob` > 0.  Needs no GPU."""
    dc = config.get("data_config") or {}
    bf = dc.get("beamform")
    if bf is None or bf is False:
        return None
    if bf is True:
        bf = {}
    if not isinstance(bf, dict):
        raise ValueError("beamform: expected true or a mapping, got %r" % (bf,))
    for k in bf:
        if k not in CONFIG_DEFAULTS and k not in MASK_KEYS:
            raise ValueError("beamform: unknown key %r (known: %s)" % (k, ", ".join(tuple(CONFIG_DEFAULTS) + MASK_KEYS)))
    out = dict(CONFIG_DEFAULTS, **bf)
    if any(k in bf for k in MASK_KEYS):
        from . import cgmm
        out["mask"], out["cgmm_iterations"] = cgmm.cgmm_config(bf)
    n = out["n_mics"]
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_CHANNELS:
        raise ValueError("beamform: n_mics must be an integer in [1, %d], got %r" % (MAX_CHANNELS, n))
    r = out["radius"]
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(float(r)) or float(r) <= 0:
        raise ValueError("beamform: radius must be a positive number of metres, got %r" % (r,))
    _ref_arg(out["ref"], int(n), "beamform")
    _diag_load_arg(out["diag_load"], "beamform")
    for key in ("online_rir", "use_reverb"):
        if not dc.get(key):
            raise ValueError("beamform: data_config %s must be true (the array's RIRs are generated for every simulated "
                             "utterance)" % key)
    if not dc.get("simulation_prob"):
        raise ValueError("beamform: data_config simulation_prob must be > 0 (only simulated utterances have an array)")
    return out


def require_beamform_config(config, prog):
    """For the trainers: exit at start-up with a one-line message when data_config `beamform` cannot be honoured."""
    try:
        return beamform_config(config)
    except ValueError as e:
        sys.stderr.write("ERROR: %s: %s\n" % (prog, e))
        sys.exit(2)
