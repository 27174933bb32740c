"""WPE dereverberation on the device (csrc/wpe.hip): weighted prediction error, multi-channel linear
prediction per frequency bin, the step in front of a mask-based beamformer.

  wpe(spec, taps, delay, iterations, diag_load)   the iterations, nothing read back: complex64 (C, N, F) -> (C, N, F)
  wpe_power(spec)                                 lambda[t, f] = max(sum_c |Y[c, t, f]|^2 / C, 1e-10): float32 (N, F)
  wpe_correlations(spec, weight, taps, delay)     R[f] = sum_t y~ y~^H / weight (F, D, D), P[f] = sum_t y~ Y^H / weight (F, D, C)
  wpe_filter_taps(R, P, diag_load)                G = (R + (diag_load tr R / D + 1e-10) I)^-1 P in float64: complex64 (F, D, C)
  wpe_apply(spec, G, delay, with_power)           X[c, t, f] = Y[c, t, f] - sum_d conj(G[f, d, c]) y~(t)[d]
  Dereverberator(analyzer, taps, delay, iterations, diag_load)     wav (C, n) or (n,) -> the same shape

y~(t)[k C + c] = Y[c, t - delay - k, f] is the stacked past, D = C taps its order.  Spectra are complex64 (C, N, F) as
SpectrumAnalyzer.analyze returns them for a (C, n) signal; C <= 8, D <= 80, 1 <= delay <= 8, 1 <= iterations <= 8.  Every
function also takes lists, one entry per utterance of a ragged minibatch (common C and F), and then makes one launch per
stage for the list.  A bin whose correlations are not finite (or not positive definite) gets G = 0 and passes through; the
flag of that stays in the device tensor `last_nonfinite`, which the library never reads.

  wpe_config(config) / require_wpe_config(config, prog)     the data_config key `wpe` (needs no GPU)
"""
import sys

import numpy as np
import torch

from . import _lib
from ._array import _as_list, _check_specs, _diag_load_arg, _frames, _int_arg, _table, analyze_channels

MAX_CHANNELS, MAX_ORDER = _lib.WPE_MAX_CHANNELS, _lib.WPE_MAX_ORDER
MAX_DELAY, MAX_ITERS = _lib.WPE_MAX_DELAY, _lib.WPE_MAX_ITERS
FRAMES_PER_PART = _lib.WPE_FRAMES_PER_PART      # frames per float32 chain of the correlation pass
CONFIG_DEFAULTS = dict(taps=10, delay=3, iterations=3, diag_load=0.001)

last_nonfinite = None      # CUDA int32 (B,) of the last wpe / wpe_filter_taps call: 1 where an utterance had a non-finite bin


def _check_params(who, taps, delay, iterations=1, diag_load=0.0, channels=None):
    taps = _int_arg(taps, 1, MAX_ORDER, who, "taps")
    delay = _int_arg(delay, 1, MAX_DELAY, who, "delay")
    iterations = _int_arg(iterations, 1, MAX_ITERS, who, "iterations")
    diag_load = _diag_load_arg(diag_load, who)
    if channels is not None:
        if channels > MAX_CHANNELS:
            raise ValueError("%s: %d channels, at most %d" % (who, channels, MAX_CHANNELS))
        if channels * taps > MAX_ORDER:
            raise ValueError("%s: %d channels x %d taps is order %d, at most %d" % (who, channels, taps, channels * taps, MAX_ORDER))
    return taps, delay, iterations, diag_load


def _workspace(frames, Cn, F, taps, delay, dev):
    nbytes = _lib.lib().pk2_wpe_workspace_bytes(_frames(frames), len(frames), Cn, F, taps, delay)
    if nbytes == 0:
        raise ValueError("wpe: no workspace for B %d, C %d, F %d, taps %d, delay %d" % (len(frames), Cn, F, taps, delay))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def wpe(spec, taps=10, delay=3, iterations=3, diag_load=1e-3):
    """spec: complex64 (C, N, F), or a list of them (one launch per stage and iteration for the list).  Returns the
    dereverberated spectra, new tensors of the same shapes.  `last_nonfinite` (CUDA int32, one entry per utterance) tells
    whether a bin of any iteration passed through for a non-finite value; it is not read back here."""
    global last_nonfinite
    specs, many, Cn, F, dev = _check_specs(spec, "wpe", MAX_CHANNELS)
    taps, delay, iterations, diag_load = _check_params("wpe", taps, delay, iterations, diag_load, Cn)
    _lib.require_gpu()
    frames = [int(s.shape[1]) for s in specs]
    outs = [torch.empty_like(s) for s in specs]
    flag = torch.empty(len(specs), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, taps, delay, dev)
        _lib.check(_lib.lib().pk2_wpe(_table(specs), _frames(frames), len(specs), Cn, F, taps, delay, iterations, diag_load,
                                      _lib.ptr(work), nbytes, _table(outs), _lib.ptr(flag), _lib.stream_ptr(dev)))
    last_nonfinite = flag
    return outs if many else outs[0]


def wpe_power(spec):
    """complex64 (C, N, F) -> float32 (N, F): the mean power over the channels, floored at 1e-10; lists -> a list."""
    specs, many, Cn, F, dev = _check_specs(spec, "wpe_power", MAX_CHANNELS)
    _lib.require_gpu()
    frames = [int(s.shape[1]) for s in specs]
    outs = [torch.empty(n, F, dtype=torch.float32, device=dev) for n in frames]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_wpe_power(_table(specs), _frames(frames), len(specs), Cn, F, _table(outs), _lib.stream_ptr(dev)))
    return outs if many else outs[0]


def wpe_correlations(spec, weight, taps=10, delay=3):
    """spec: complex64 (C, N, F); weight: float32 (N, F), applied as its reciprocal (wpe_power's lambda).  Returns
    (R complex64 (F, D, D), exactly Hermitian, P complex64 (F, D, C)); lists -> (list of R, list of P), one launch."""
    specs, many, Cn, F, dev = _check_specs(spec, "wpe_correlations", MAX_CHANNELS)
    taps, delay, _, _ = _check_params("wpe_correlations", taps, delay, channels=Cn)
    ws = list(weight) if many else [weight]
    if len(ws) != len(specs):
        raise ValueError("wpe_correlations: %d spectra, %d weights" % (len(specs), len(ws)))
    for i, (s, w) in enumerate(zip(specs, ws)):
        if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.device == dev
                and tuple(w.shape) == (s.shape[1], F)):
            raise ValueError("wpe_correlations: utterance %d: weight must be a contiguous CUDA float32 (N, F) = (%d, %d) tensor "
                             "on %s" % (i, s.shape[1], F, dev))
    _lib.require_gpu()
    frames, B, D = [int(s.shape[1]) for s in specs], len(specs), Cn * taps
    R = torch.empty(B, F, D, D, dtype=torch.complex64, device=dev)
    P = torch.empty(B, F, D, Cn, dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, taps, delay, dev)
        _lib.check(_lib.lib().pk2_wpe_corr(_table(specs), _table(ws), _frames(frames), B, Cn, F, taps, delay, _lib.ptr(work), nbytes,
                                           _lib.ptr(R), _lib.ptr(P), _lib.stream_ptr(dev)))
    return (list(R.unbind(0)), list(P.unbind(0))) if many else (R[0], P[0])


def wpe_filter_taps(R, P, diag_load=1e-3):
    """R: complex64 (F, D, D), P: complex64 (F, D, C) -> G complex64 (F, D, C), solved in float64 on the device; lists -> a
    list.  Sets `last_nonfinite`."""
    global last_nonfinite
    Rs, many = _as_list(R, "wpe_filter_taps")
    Ps = list(P) if many else [P]
    if len(Ps) != len(Rs):
        raise ValueError("wpe_filter_taps: %d matrices R, %d matrices P" % (len(Rs), len(Ps)))
    for i, (r, p) in enumerate(zip(Rs, Ps)):
        for what, x in (("R", r), ("P", p)):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.complex64 and x.dim() == 3 and x.numel() > 0):
                raise ValueError("wpe_filter_taps: utterance %d: %s must be a CUDA complex64 tensor of three dimensions" % (i, what))
        if r.shape[1] != r.shape[2] or tuple(p.shape[:2]) != tuple(r.shape[:2]) or r.shape != Rs[0].shape or p.shape != Ps[0].shape \
                or r.device != Rs[0].device or p.device != Rs[0].device:
            raise ValueError("wpe_filter_taps: utterance %d: R %r and P %r must be (F, D, D) and (F, D, C), the same for every "
                             "utterance and on one device" % (i, tuple(r.shape), tuple(p.shape)))
    F, D, Cn, dev = Rs[0].shape[0], Rs[0].shape[1], Ps[0].shape[2], Rs[0].device
    if Cn > MAX_CHANNELS or D > MAX_ORDER or D % Cn:
        raise ValueError("wpe_filter_taps: order %d on %d channels (C <= %d, D = C taps <= %d)" % (D, Cn, MAX_CHANNELS, MAX_ORDER))
    diag_load = _diag_load_arg(diag_load, "wpe_filter_taps")
    _lib.require_gpu()
    B = len(Rs)
    Rc, Pc = torch.stack(Rs).contiguous(), torch.stack(Ps).contiguous()
    G = torch.empty(B, F, D, Cn, dtype=torch.complex64, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(max(256, B * F * 4 + 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_wpe_solve(_lib.ptr(Rc), _lib.ptr(Pc), B, Cn, F, D // Cn, diag_load, _lib.ptr(work), work.numel(),
                                            _lib.ptr(G), _lib.ptr(flag), _lib.stream_ptr(dev)))
    last_nonfinite = flag
    return list(G.unbind(0)) if many else G[0]


def wpe_apply(spec, G, delay=3, with_power=False):
    """spec: complex64 (C, N, F); G: complex64 (F, D, C).  Returns X complex64 (C, N, F), a new tensor, and with
    with_power=True (X, wpe_power(X)) from the same pass; lists -> lists."""
    specs, many, Cn, F, dev = _check_specs(spec, "wpe_apply", MAX_CHANNELS)
    Gs = list(G) if many else [G]
    if len(Gs) != len(specs):
        raise ValueError("wpe_apply: %d spectra, %d filters" % (len(specs), len(Gs)))
    for i, g in enumerate(Gs):
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.complex64 and g.dim() == 3 and g.device == dev
                and g.shape[0] == F and g.shape[2] == Cn and g.shape == Gs[0].shape and g.shape[1] % Cn == 0 and g.shape[1] > 0):
            raise ValueError("wpe_apply: utterance %d: G must be a CUDA complex64 (F, D, C) = (%d, C taps, %d) tensor on %s"
                             % (i, F, Cn, dev))
    taps, delay, _, _ = _check_params("wpe_apply", Gs[0].shape[1] // Cn, delay, channels=Cn)
    _lib.require_gpu()
    frames, B = [int(s.shape[1]) for s in specs], len(specs)
    Gc = torch.stack(Gs).contiguous()
    outs = [torch.empty_like(s) for s in specs]
    pows = [torch.empty(n, F, dtype=torch.float32, device=dev) for n in frames] if with_power else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_wpe_filter(_table(specs), _lib.ptr(Gc), _frames(frames), B, Cn, F, taps, delay, _table(outs),
                                             _table(pows) if with_power else None, _lib.stream_ptr(dev)))
    if with_power:
        return (outs, pows) if many else (outs[0], pows[0])
    return outs if many else outs[0]


class Dereverberator:
    """analyzer: a simulation.SpectrumAnalyzer (its FFT size, frame and window; the analysis here never dithers, whatever
    the analyzer's do_dither).  __call__(wav): (C, n) or (n,) CUDA float32 -> the same shape: STFT, wpe, inverse STFT cut to
    n.  `batch` does it for a ragged list with one launch per WPE stage (the STFT entries take one length per call);
    `spectrum` is wpe() with this object's parameters, for callers that stay in the STFT domain.  `last_nonfinite` (CUDA
    int32, one entry per utterance) keeps the last call's flag and is not read back."""

    def __init__(self, analyzer, taps=10, delay=3, iterations=3, diag_load=1e-3):
        self.analyzer = analyzer
        self.taps, self.delay, self.iterations, self.diag_load = _check_params("Dereverberator", taps, delay, iterations, diag_load)
        self.last_nonfinite = None

    def analyze(self, wav):
        """(C, n) CUDA float32 -> complex64 (C, N, F), without dither"""
        spec = analyze_channels(self.analyzer, wav, "Dereverberator", MAX_CHANNELS)
        _check_params("Dereverberator", self.taps, self.delay, channels=spec.shape[0])
        return spec

    def spectrum(self, spec):
        out = wpe(spec, self.taps, self.delay, self.iterations, self.diag_load)
        self.last_nonfinite = last_nonfinite
        return out

    def batch(self, wavs):
        wavs = list(wavs)
        flat = [isinstance(x, torch.Tensor) and x.dim() == 1 for x in wavs]
        mc = [x.view(1, -1) if one else x for x, one in zip(wavs, flat)]
        specs = [self.analyze(x) for x in mc]
        outs = self.spectrum(specs)
        ys = [self.analyzer.synthesize(X)[:, :x.shape[1]] for X, x in zip(outs, mc)]
        return [y[0] if one else y for y, one in zip(ys, flat)]

    def __call__(self, wav):
        return self.batch([wav])[0]


def wpe_config(config):
    """data_config `wpe`: true (the defaults taps 10, delay 3, iterations 3, diag_load 0.001) or a mapping over them; None
    when the key is absent or false.  Raises ValueError for an unknown key, a bad value, an order n_mics * taps above 80 with
    `beamform`, and for a configuration that cannot honour the key: it needs `use_reverb: true` and `simulation_prob` > 0.
    Needs no GPU."""
    dc = config.get("data_config") or {}
    w = dc.get("wpe")
    if w is None or w is False:
        return None
    if w is True:
        w = {}
    if not isinstance(w, dict):
        raise ValueError("wpe: expected true or a mapping, got %r" % (w,))
    for k in w:
        if k not in CONFIG_DEFAULTS:
            raise ValueError("wpe: unknown key %r (known: %s)" % (k, ", ".join(CONFIG_DEFAULTS)))
    out = dict(CONFIG_DEFAULTS, **w)
    channels = 1
    bf = dc.get("beamform")
    if bf:
        n = bf.get("n_mics", 7) if isinstance(bf, dict) else 7
        channels = int(n) if isinstance(n, (int, np.integer)) and not isinstance(n, bool) and 1 <= n <= MAX_CHANNELS else 1
    _check_params("wpe", out["taps"], out["delay"], out["iterations"], out["diag_load"], channels)
    if not dc.get("use_reverb"):
        raise ValueError("wpe: data_config use_reverb must be true (there is no reverberation to remove otherwise)")
    if not dc.get("simulation_prob"):
        raise ValueError("wpe: data_config simulation_prob must be > 0 (only simulated utterances are dereverberated)")
    return out


def require_wpe_config(config, prog):
    """For the trainers: exit at start-up with a one-line message when data_config `wpe` cannot be honoured."""
    try:
        return wpe_config(config)
    except ValueError as e:
        sys.stderr.write("ERROR: %s: %s\n" % (prog, e))
        sys.exit(2)
