"""cGMM mask estimation on the device (csrc/cgmm.hip): the unsupervised time-frequency masks a mask-based
beamformer needs on a recording, where no clean source exists for simulation.MaskEstimator's ideal mask.  Per frequency bin
an EM over the frames of a mixture of K complex Gaussians y ~ N(0, phi_k[t] R_k) with weights alpha_k (Higuchi et al.
2016); with a per-class frame activity it is the guided form used for overlapped speech.

  cgmm_masks(spec, num_classes, iterations, init, activity, diag_load, order, seed)   the whole EM: float32 masks (K, N, F)
  cgmm_init(spec, init, activity)              the start state (R complex64 (K, F, C, C), log_alpha float32 (K, F))
  cgmm_factor(R, log_alpha, diag_load)         R' = L L^H in float64: (L^-1 planes, b = log alpha - 2 sum log L_jj, bad)
  cgmm_posteriors(spec, factor, activity)      (lambda (K, N, F), phi (K, N, F), log-likelihood float64 ())
  cgmm_update(spec, lam, phi, activity)        the M-step: (R, log_alpha)
  CgmmMaskEstimator(analyzer, iterations, diag_load)      wav (C, n) -> (speech mask, noise mask), for MaskBeamformer

Spectra are complex64 (C, N, F) as MaskBeamformer.analyze returns them; 1 <= C <= 8, 2 <= K <= 4, 1 <= iterations <= 32.
`init` is K masks (a (K, N, F) tensor or K tensors (N, F)); without it K = 2 and class 0 starts from the observed
covariance, class 1 from a scaled identity.  init='random' is the blind start for any K: seeded uniform masks drawn on the
host (random_init(K, N, F, seed, i) for utterance i of the call), in the order 'keep': the classes of different bins are then
unrelated, and pykaldi2_amd.separate.align_permutations puts them in one order.  `activity` is float32 (K, N), >= 0: a
class with activity 0 on a frame gets a zero mask there.  order='purity' (K = 2, the default without `init`) makes class 0,
bin by bin, the class whose covariance is closer to rank one: the directional source; 'keep' (the default with `init`)
leaves the classes as they are.  Every function
also takes lists, one entry per utterance of a ragged minibatch (common C, F and K), and then makes one launch per stage for
the list.  `last_ll` (float64 (iterations,), or (B, iterations)), `last_cov` ((K, F, C, C): the M-step of the returned
masks), `last_log_alpha` and `last_nonfinite` (int32, one entry per utterance: a bin was not finite or not positive definite
and got the masks 1 / K) keep the last cgmm_masks call's; they are device tensors the library never reads.

  cgmm_config(beamform_config)      validation of the data_config keys `beamform: {mask, cgmm_iterations}` (needs no GPU)
"""
import numpy as np
import torch

from . import _lib
from ._array import _as_list, _check_specs, _diag_load_arg, _frames, _int_arg, _table, analyze_channels

MAX_CHANNELS, MAX_CLASSES, MAX_ITERS = _lib.BF_MAX_CHANNELS, _lib.BF_MAX_MASKS, _lib.CGMM_MAX_ITERS
MASK_KINDS = ("ideal", "cgmm")

last_ll = last_cov = last_log_alpha = last_nonfinite = None


def _per_utt(x, many, n, who, name):
    if x is None:
        return None
    xs = list(x) if many else [x]
    if len(xs) != n:
        raise ValueError("%s: %d spectra, %d entries of %s" % (who, n, len(xs), name))
    return xs


def _planes(x, specs, K, who, name):
    """one (K, N, F) float32 tensor per utterance; K is taken from the first when None"""
    out = []
    for i, (s, p) in enumerate(zip(specs, x)):
        if isinstance(p, (list, tuple)):
            if not p or not all(isinstance(q, torch.Tensor) and q.dim() == 2 for q in p):
                raise ValueError("%s: utterance %d: %s must be a (K, N, F) tensor or K tensors (N, F)" % (who, i, name))
            if any(q.shape != p[0].shape or q.dtype != p[0].dtype or q.device != p[0].device for q in p):
                raise ValueError("%s: utterance %d: the %d tensors of %s differ in shape, dtype or device" % (who, i, len(p), name))
            p = torch.stack(list(p))
        if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 and p.dim() == 3 and p.device == s.device):
            raise ValueError("%s: utterance %d: %s must be CUDA float32 (K, N, F) on %s" % (who, i, name, s.device))
        K = p.shape[0] if K is None else K
        if tuple(p.shape) != (K, s.shape[1], s.shape[2]):
            raise ValueError("%s: utterance %d: %s has shape %r, expected (K, N, F) = (%d, %d, %d)"
                             % (who, i, name, tuple(p.shape), K, s.shape[1], s.shape[2]))
        out.append(p.contiguous())
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError("%s: %d classes (2 to %d)" % (who, K, MAX_CLASSES))
    return out, K


def _activity(activity, specs, many, K, who):
    acts = _per_utt(activity, many, len(specs), who, "activity")
    if acts is None:
        return None
    out = []
    for i, (s, a) in enumerate(zip(specs, acts)):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.device == s.device
                and tuple(a.shape) == (K, s.shape[1])):
            raise ValueError("%s: utterance %d: activity must be CUDA float32 (K, N) = (%d, %d) on %s"
                             % (who, i, K, s.shape[1], s.device))
        out.append(a.contiguous())
    return out


def _workspace(frames, Cn, F, K, dev):
    nbytes = _lib.lib().pk2_cgmm_workspace_bytes(_frames(frames), len(frames), Cn, F, K)
    if nbytes == 0:
        raise ValueError("cgmm: no workspace for B %d, C %d, F %d, K %d" % (len(frames), Cn, F, K))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _order_arg(order, init, K, who):
    if order is None:
        order = "purity" if init is None else "keep"
    if order not in ("purity", "keep"):
        raise ValueError("%s: order must be 'purity' or 'keep', got %r" % (who, order))
    if order == "purity" and K != 2:
        raise ValueError("%s: order='purity' is defined for two classes, not %d" % (who, K))
    return order == "purity"


def random_init(K, N, F, seed, index=0):
    """The blind start of cgmm_masks(init='random', seed) for utterance `index` of a call: numpy float32 (K, N, F), uniform
    draws of numpy.random.default_rng([seed, index]) plus 0.05, normalised over the classes.  Needs no GPU."""
    x = np.random.default_rng([seed, index]).random((K, N, F), np.float32) + np.float32(0.05)
    return (x / x.sum(axis=0, keepdims=True)).astype(np.float32)


def cgmm_masks(spec, num_classes=2, iterations=10, init=None, activity=None, diag_load=1e-3, order=None, seed=0):
    """spec: complex64 (C, N, F), or a list of them (one launch per stage and iteration for the list).  Returns float32
    (K, N, F): the posteriors of the last E-step; for a list, a list.  See the module text for the arguments and for
    `last_ll`, `last_cov`, `last_log_alpha` and `last_nonfinite`.  Nothing is read back."""
    global last_ll, last_cov, last_log_alpha, last_nonfinite
    who = "cgmm_masks"
    specs, many, Cn, F, dev = _check_specs(spec, who, MAX_CHANNELS)
    K = _int_arg(num_classes, 2, MAX_CLASSES, who, "num_classes")
    iterations = _int_arg(iterations, 1, MAX_ITERS, who, "iterations")
    diag_load = _diag_load_arg(diag_load, who)
    if isinstance(init, str):
        if init != "random":
            raise ValueError("%s: init must be masks or 'random', got %r" % (who, init))
        seed = _int_arg(seed, 0, 2 ** 63 - 1, who, "seed")
        draws = [_lib.h2d(random_init(K, int(s.shape[1]), F, seed, i), dev) for i, s in enumerate(specs)]
        init = draws if many else draws[0]
    inits = _per_utt(init, many, len(specs), who, "init")
    if inits is not None:
        inits, Ki = _planes(inits, specs, None, who, "init")
        if Ki != K:
            raise ValueError("%s: init has %d masks, num_classes is %d" % (who, Ki, K))
    elif K != 2:
        raise ValueError("%s: %d classes need init (without it there are two: the source and the noise)" % (who, K))
    purity = _order_arg(order, init, K, who)
    acts = _activity(activity, specs, many, K, who)
    _lib.require_gpu()
    frames, B = [int(s.shape[1]) for s in specs], len(specs)
    masks = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    R = torch.empty(B, K, F, Cn, Cn, dtype=torch.complex64, device=dev)
    la = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    ll = torch.empty(B, iterations, dtype=torch.float64, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, K, dev)
        _lib.check(_lib.lib().pk2_cgmm(_table(specs), _table(inits) if inits else None, _table(acts) if acts else None,
                                       _frames(frames), B, Cn, F, K, iterations, diag_load, int(purity), _lib.ptr(work), nbytes,
                                       _table(masks), _lib.ptr(R), _lib.ptr(la), _lib.ptr(ll), _lib.ptr(flag),
                                       _lib.stream_ptr(dev)))
    last_nonfinite = flag
    if many:
        last_ll, last_cov, last_log_alpha = ll, list(R.unbind(0)), list(la.unbind(0))
        return masks
    last_ll, last_cov, last_log_alpha = ll[0], R[0], la[0]
    return masks[0]


def cgmm_init(spec, init=None, activity=None):
    """The start state (R complex64 (K, F, C, C), log_alpha float32 (K, F)); lists -> (list of R, list of log_alpha).
    Without `init`, K = 2: R_0 = sum_t y y^H / N, R_1 = (Re tr R_0 / C) I, alpha = 1 / 2; with it, cgmm_update with
    lam = init and phi = 1."""
    who = "cgmm_init"
    specs, many, Cn, F, dev = _check_specs(spec, who, MAX_CHANNELS)
    inits, K = _per_utt(init, many, len(specs), who, "init"), 2
    if inits is not None:
        inits, K = _planes(inits, specs, None, who, "init")
    acts = _activity(activity, specs, many, K, who)
    _lib.require_gpu()
    frames, B = [int(s.shape[1]) for s in specs], len(specs)
    R = torch.empty(B, K, F, Cn, Cn, dtype=torch.complex64, device=dev)
    la = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, K, dev)
        _lib.check(_lib.lib().pk2_cgmm_init(_table(specs), _table(inits) if inits else None, _table(acts) if acts else None,
                                            _frames(frames), B, Cn, F, K, _lib.ptr(work), nbytes, _lib.ptr(R), _lib.ptr(la),
                                            _lib.stream_ptr(dev)))
    return (list(R.unbind(0)), list(la.unbind(0))) if many else (R[0], la[0])


def _check_state(R, log_alpha, who):
    Rs, many = _as_list(R, who)
    las = list(log_alpha) if many else [log_alpha]
    if len(las) != len(Rs):
        raise ValueError("%s: %d covariances, %d entries of log_alpha" % (who, len(Rs), len(las)))
    for i, (r, a) in enumerate(zip(Rs, las)):
        if not (isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.complex64 and r.dim() == 4
                and r.shape[2] == r.shape[3] and r.numel() > 0 and r.shape == Rs[0].shape and r.device == Rs[0].device):
            raise ValueError("%s: utterance %d: R must be a CUDA complex64 (K, F, C, C) tensor, the same shape for every "
                             "utterance" % (who, i))
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.device == r.device
                and tuple(a.shape) == tuple(r.shape[:2])):
            raise ValueError("%s: utterance %d: log_alpha must be CUDA float32 (K, F) = (%d, %d) on %s"
                             % (who, i, r.shape[0], r.shape[1], r.device))
    K, F, Cn = Rs[0].shape[0], Rs[0].shape[1], Rs[0].shape[2]
    if Cn > MAX_CHANNELS or not 2 <= K <= MAX_CLASSES:
        raise ValueError("%s: %d classes on %d channels (2 to %d classes, at most %d channels)"
                         % (who, K, Cn, MAX_CLASSES, MAX_CHANNELS))
    return Rs, las, many, K, F, Cn, Rs[0].device


def cgmm_factor(R, log_alpha, diag_load=1e-3):
    """R: complex64 (K, F, C, C), log_alpha: float32 (K, F).  Returns the factor (linv float32 (K, C (C + 1), F): the lower
    triangle of L^-1 row by row as (re, im) planes over the bins; bias float32 (K, F); bad int32 (K, F)), factored in
    float64 on the device; lists -> a list of factors.  Sets `last_nonfinite`."""
    global last_nonfinite
    who = "cgmm_factor"
    Rs, las, many, K, F, Cn, dev = _check_state(R, log_alpha, who)
    diag_load = _diag_load_arg(diag_load, who)
    _lib.require_gpu()
    B = len(Rs)
    Rc, lac = torch.stack(Rs).contiguous(), torch.stack(las).contiguous()
    linv = torch.empty(B, K, Cn * (Cn + 1), F, dtype=torch.float32, device=dev)
    bias = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    bad = torch.empty(B, K, F, dtype=torch.int32, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_cgmm_factor(_lib.ptr(Rc), _lib.ptr(lac), B, Cn, F, K, diag_load, _lib.ptr(linv), _lib.ptr(bias),
                                              _lib.ptr(bad), _lib.ptr(flag), _lib.stream_ptr(dev)))
    last_nonfinite = flag
    out = [(linv[b], bias[b], bad[b]) for b in range(B)]
    return out if many else out[0]


def cgmm_posteriors(spec, factor, activity=None):
    """spec: complex64 (C, N, F); factor: what cgmm_factor returned.  Returns (lam float32 (K, N, F), phi float32 (K, N, F),
    ll float64 (): the log-likelihood up to its constant); lists -> (list, list, ll (B,))."""
    who = "cgmm_posteriors"
    specs, many, Cn, F, dev = _check_specs(spec, who, MAX_CHANNELS)
    facs = list(factor) if many else [factor]
    if len(facs) != len(specs):
        raise ValueError("%s: %d spectra, %d factors" % (who, len(specs), len(facs)))
    K = None
    for i, fac in enumerate(facs):
        if not (isinstance(fac, (tuple, list)) and len(fac) == 3 and all(isinstance(x, torch.Tensor) and x.is_cuda for x in fac)):
            raise ValueError("%s: utterance %d: the factor must be the three CUDA tensors of cgmm_factor" % (who, i))
        linv, bias, bad = fac
        K = bias.shape[0] if K is None and bias.dim() == 2 else K
        if linv.dtype != torch.float32 or bias.dtype != torch.float32 or bad.dtype != torch.int32 \
                or tuple(linv.shape) != (K, Cn * (Cn + 1), F) or tuple(bias.shape) != (K, F) or tuple(bad.shape) != (K, F) \
                or any(x.device != dev for x in fac):
            raise ValueError("%s: utterance %d: the factor does not fit (K, C, F) = (%r, %d, %d) on %s" % (who, i, K, Cn, F, dev))
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError("%s: %d classes (2 to %d)" % (who, K, MAX_CLASSES))
    acts = _activity(activity, specs, many, K, who)
    _lib.require_gpu()
    frames, B = [int(s.shape[1]) for s in specs], len(specs)
    linv = torch.stack([f[0] for f in facs]).contiguous()
    bias = torch.stack([f[1] for f in facs]).contiguous()
    bad = torch.stack([f[2] for f in facs]).contiguous()
    lam = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    phi = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    ll = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, K, dev)
        _lib.check(_lib.lib().pk2_cgmm_posteriors(_table(specs), _table(acts) if acts else None, _frames(frames), B, Cn, F, K,
                                                  _lib.ptr(linv), _lib.ptr(bias), _lib.ptr(bad), _lib.ptr(work), nbytes,
                                                  _table(lam), _table(phi), _lib.ptr(ll), _lib.stream_ptr(dev)))
    return (lam, phi, ll) if many else (lam[0], phi[0], ll[0])


def cgmm_update(spec, lam, phi, activity=None):
    """The M-step: R_k[f] = sum_t (lam_k / phi_k) y y^H / max(sum_t lam_k, 1e-10), exactly Hermitian, and
    log alpha_k[f] = log max(sum_t lam_k / N_act, 1e-10), N_act the number of frames with an active class (all of them
    without `activity`).  Returns (R complex64 (K, F, C, C), log_alpha float32 (K, F)); lists -> lists."""
    who = "cgmm_update"
    specs, many, Cn, F, dev = _check_specs(spec, who, MAX_CHANNELS)
    lams, K = _planes(_per_utt(lam, many, len(specs), who, "lam"), specs, None, who, "lam")
    phis, _ = _planes(_per_utt(phi, many, len(specs), who, "phi"), specs, K, who, "phi")
    acts = _activity(activity, specs, many, K, who)
    _lib.require_gpu()
    frames, B = [int(s.shape[1]) for s in specs], len(specs)
    R = torch.empty(B, K, F, Cn, Cn, dtype=torch.complex64, device=dev)
    la = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        work, nbytes = _workspace(frames, Cn, F, K, dev)
        _lib.check(_lib.lib().pk2_cgmm_update(_table(specs), _table(lams), _table(phis), _table(acts) if acts else None,
                                              _frames(frames), B, Cn, F, K, _lib.ptr(work), nbytes, _lib.ptr(R), _lib.ptr(la),
                                              _lib.stream_ptr(dev)))
    return (list(R.unbind(0)), list(la.unbind(0))) if many else (R[0], la[0])


class CgmmMaskEstimator:
    """analyzer: a simulation.SpectrumAnalyzer (its FFT size, frame and window; the analysis here never dithers).
    __call__(wav (C, n)) -> (speech_mask, noise_mask), float32 (N, F) each: STFT, then `masks`.  masks(spec): two-class
    cgmm_masks in the purity order, so the first mask is the directional source's, for callers already in the STFT domain; a
    list of spectra gives a list of pairs from one launch per stage.  `batch(wavs)` does that for a ragged list of
    waveforms.  `last_ll`, `last_cov` and `last_nonfinite` keep the last call's device tensors."""

    def __init__(self, analyzer, iterations=10, diag_load=1e-3):
        self.analyzer = analyzer
        self.iterations = _int_arg(iterations, 1, MAX_ITERS, "CgmmMaskEstimator", "iterations")
        self.diag_load = _diag_load_arg(diag_load, "CgmmMaskEstimator")
        self.last_ll = self.last_cov = self.last_nonfinite = None

    def analyze(self, wav):
        """(C, n) CUDA float32 -> complex64 (C, N, F), without dither"""
        return analyze_channels(self.analyzer, wav, "CgmmMaskEstimator", MAX_CHANNELS)

    def masks(self, spec):
        m = cgmm_masks(spec, 2, self.iterations, diag_load=self.diag_load)
        self.last_ll, self.last_cov, self.last_nonfinite = last_ll, last_cov, last_nonfinite
        if isinstance(spec, (list, tuple)):
            return [(x[0], x[1]) for x in m]
        return m[0], m[1]

    def batch(self, wavs):
        return self.masks([self.analyze(x) for x in wavs])

    def __call__(self, wav):
        return self.masks(self.analyze(wav))


FRONT_ENDS = ("none", "mvdr", "wpe_mvdr", "sep_mvdr", "wpe_sep_mvdr")


class ArrayFrontEnd:
    """The multi-channel front end of a recording (bin/dump_loglikes.py -array_frontend): kind 'mvdr': cGMM masks -> MVDR;
    'wpe_mvdr': WPE on the array spectrum first.  __call__(wavs): a list of (C, n) CUDA float32 signals (common C) -> a
    list of (n,) enhanced waveforms; one forward and one inverse transform per utterance, and between them one launch per
    stage for the whole list.  A one-channel signal has nothing to beamform and comes back as it is.  The kinds 'sep_mvdr'
    and 'wpe_sep_mvdr' separate overlapped speech (pykaldi2_amd.separate): blind cGMM masks for num_speakers speakers and
    the noise, aligned over the bins, and one MVDR beamformer per speaker; the result is then a list of num_speakers
    waveforms per recording (a one-channel signal comes back once, as a list of one)."""

    def __init__(self, kind, analyzer=None, iterations=None, ref=0, diag_load=1e-3, wpe=None, num_speakers=2, seed=0):
        from . import beamform, dereverb, simulation
        if kind not in FRONT_ENDS[1:]:
            raise ValueError("ArrayFrontEnd: kind must be one of %s, got %r" % (" | ".join(FRONT_ENDS[1:]), kind))
        self.kind = kind
        self.separates = kind in ("sep_mvdr", "wpe_sep_mvdr")
        if self.separates:
            self.num_speakers = _int_arg(num_speakers, 1, MAX_CLASSES - 1, "ArrayFrontEnd", "num_speakers")
        self.analyzer = analyzer if analyzer is not None else simulation.SpectrumAnalyzer(do_dither=False)
        self.beamformer = beamform.MaskBeamformer(self.analyzer, ref, diag_load)
        if self.separates:
            from . import separate
            self.estimator = separate.CgmmSeparator(self.analyzer, self.num_speakers, 20 if iterations is None else iterations,
                                                    seed=seed)
        else:
            self.estimator = CgmmMaskEstimator(self.analyzer, 10 if iterations is None else iterations)
        self.dereverb = dereverb.Dereverberator(self.analyzer, **(wpe or {})) if kind.startswith("wpe_") else None

    def __call__(self, wavs):
        from . import beamform
        wavs = list(wavs)
        if all(x.shape[0] == 1 for x in wavs):
            return [[x[0]] for x in wavs] if self.separates else [x[0] for x in wavs]
        specs = [self.beamformer.analyze(x) for x in wavs]
        if self.dereverb is not None:
            specs = self.dereverb.spectrum(specs)
        if self.separates:
            from . import separate
            streams = separate.separate(specs, self.estimator.masks(specs), self.beamformer.ref, self.beamformer.diag_load)
            return [[self.analyzer.synthesize(X)[:x.shape[1]] for X in st] for st, x in zip(streams, wavs)]
        phi = beamform.spatial_covariance(specs, [list(p) for p in self.estimator.masks(specs)])
        w, _ = beamform.mvdr_weights([p[0] for p in phi], [p[1] for p in phi], self.beamformer.ref, self.beamformer.diag_load)
        enhanced = beamform.apply_weights(specs, w)
        return [self.analyzer.synthesize(X)[:x.shape[1]] for X, x in zip(enhanced, wavs)]


def cgmm_config(bf):
    """bf: the mapping of data_config `beamform` (or True / None).  Returns (mask, cgmm_iterations): mask 'ideal' (the
    default: the ideal mask of the simulated source) or 'cgmm' (estimated from the array spectrum), cgmm_iterations 10 by
    default.  Raises ValueError for a bad value.  Needs no GPU."""
    bf = bf if isinstance(bf, dict) else {}
    mask, iters = bf.get("mask", "ideal"), bf.get("cgmm_iterations", 10)
    if mask not in MASK_KINDS:
        raise ValueError("beamform: mask must be one of %s, got %r" % (" | ".join(MASK_KINDS), mask))
    return mask, _int_arg(iters, 1, MAX_ITERS, "beamform", "cgmm_iterations")
