"""Blind speaker separation on the device (csrc/perm_align.hip): one stream per speaker from an array
recording of overlapped speech, with no initial masks and no activity.  A blind cGMM (cgmm.cgmm_masks(init='random')) runs
per frequency bin, so its classes are unrelated from bin to bin; the aligner matches the bins by how their posteriors move
over time (Sawada et al. 2011), and every speaker gets its own MVDR beamformer.

  align_permutations(masks, cov, log_alpha, refine, noise_last)     aligned masks (and cov, log_alpha): float32 (K, N, F)
  CgmmSeparator(analyzer, num_speakers, iterations, refine, seed)   masks(specs) -> (S + 1, N, F): speakers first, noise last
  separate(specs, masks, ref, diag_load)                            S spectra (N, F) per utterance, MVDR per speaker

Masks are float32 (K, N, F), 2 <= K <= 4, as cgmm_masks returns them; `cov` complex64 (K, F, C, C) and `log_alpha` float32
(K, F) are cgmm.last_cov and cgmm.last_log_alpha.  Every function also takes lists, one entry per utterance of a ragged
minibatch (common K, F and C), and then makes one launch per stage for the list.  `last_perm` (int32 (F, K): the aligned
class a of bin f is the input's class last_perm[f, a]) and `last_margin` (float32 (F,): the best assignment's score minus
the second best's in the last refinement round) keep the last align_permutations call's; for a list they are (B, F, K) and
(B, F).  They are device tensors the library never reads.  Two speakers are what the tests and DESIGN.md 7.12 speak of; three
blind speakers (K = 4) are allowed and not promised.
"""
import torch

from . import _lib, beamform, cgmm
from ._array import _as_list, _check_specs, _diag_load_arg, _frames, _int_arg, _table

MAX_CLASSES, MAX_REFINE = _lib.BF_MAX_MASKS, _lib.PERM_ALIGN_MAX_REFINE
MAX_SPEAKERS = MAX_CLASSES - 1

last_perm = last_margin = None


def _check_masks(masks, who):
    ms, many = _as_list(masks, who)
    for i, m in enumerate(ms):
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 3 and m.numel() > 0):
            raise ValueError("%s: utterance %d: masks must be a CUDA float32 (K, N, F) tensor" % (who, i))
        if m.shape[0] != ms[0].shape[0] or m.shape[2] != ms[0].shape[2] or m.device != ms[0].device:
            raise ValueError("%s: utterance %d is (K, F) = (%d, %d) on %s, the first one (%d, %d) on %s"
                             % (who, i, m.shape[0], m.shape[2], m.device, ms[0].shape[0], ms[0].shape[2], ms[0].device))
    K, F = ms[0].shape[0], ms[0].shape[2]
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError("%s: %d classes (2 to %d)" % (who, K, MAX_CLASSES))
    if F > 4097:
        raise ValueError("%s: %d bins, at most 4097" % (who, F))
    return [m.contiguous() for m in ms], many, K, F, ms[0].device


def align_permutations(masks, cov=None, log_alpha=None, refine=3, noise_last=True):
    """masks: float32 (K, N, F), or a list (one launch per stage for the list).  Returns the aligned masks, out of place;
    with `cov` and `log_alpha` (both or neither) the tuple (masks, cov, log_alpha), gathered the same way.  noise_last (only
    with `cov`): the stream whose covariances are, summed over the bins, the furthest from rank one moves to position
    K - 1.  Sets `last_perm` and `last_margin`.  Bad arguments raise ValueError before any launch; nothing is read back."""
    global last_perm, last_margin
    who = "align_permutations"
    ms, many, K, F, dev = _check_masks(masks, who)
    refine = _int_arg(refine, 1, MAX_REFINE, who, "refine")
    if not isinstance(noise_last, bool):
        raise ValueError("%s: noise_last must be True or False, got %r" % (who, noise_last))
    if (cov is None) != (log_alpha is None):
        raise ValueError("%s: cov and log_alpha are given together or not at all" % who)
    B, Cn, Rc, lac = len(ms), 0, None, None
    if cov is not None:
        if isinstance(cov, (list, tuple)) != many or isinstance(log_alpha, (list, tuple)) != many:
            raise ValueError("%s: masks, cov and log_alpha are all tensors or all lists" % who)
        Rs, las, _, Kc, Fc, Cn, devc = cgmm._check_state(cov, log_alpha, who)
        if len(Rs) != B or Kc != K or Fc != F or devc != dev:
            raise ValueError("%s: %d covariances (K, F) = (%d, %d) on %s for %d masks (%d, %d) on %s"
                             % (who, len(Rs), Kc, Fc, devc, B, K, F, dev))
        Rc, lac = torch.stack(Rs).contiguous(), torch.stack(las).contiguous()
    _lib.require_gpu()
    frames = [int(m.shape[1]) for m in ms]
    out = [torch.empty_like(m) for m in ms]
    perm = torch.empty(B, F, K, dtype=torch.int32, device=dev)
    margin = torch.empty(B, F, dtype=torch.float32, device=dev)
    Ro = torch.empty_like(Rc) if Rc is not None else None
    lao = torch.empty_like(lac) if lac is not None else None
    with torch.cuda.device(dev):
        nbytes = _lib.lib().pk2_perm_align_workspace_bytes(_frames(frames), B, F, K)
        if nbytes == 0:
            raise ValueError("%s: no workspace for B %d, F %d, K %d" % (who, B, F, K))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().pk2_perm_align(_table(ms), _lib.ptr(Rc), _lib.ptr(lac), _frames(frames), B, Cn, F, K, refine,
                                             int(noise_last), _lib.ptr(work), nbytes, _table(out), _lib.ptr(Ro), _lib.ptr(lao),
                                             _lib.ptr(perm), _lib.ptr(margin), _lib.stream_ptr(dev)))
    last_perm, last_margin = (perm, margin) if many else (perm[0], margin[0])
    if Rc is None:
        return out if many else out[0]
    return (out, list(Ro.unbind(0)), list(lao.unbind(0))) if many else (out[0], Ro[0], lao[0])


class CgmmSeparator:
    """analyzer: a simulation.SpectrumAnalyzer (its FFT size, frame and window; the analysis here never dithers).
    masks(spec): blind cGMM with num_speakers + 1 classes from a seeded random start, then align_permutations on its
    covariances: float32 (num_speakers + 1, N, F), the speakers first and the noise last; a list of spectra gives a list
    from one launch per stage.  `last_ll`, `last_cov` (aligned), `last_perm`, `last_margin` and `last_nonfinite` keep the
    last call's device tensors."""

    def __init__(self, analyzer, num_speakers=2, iterations=20, refine=3, seed=0, diag_load=1e-3):
        who = "CgmmSeparator"
        self.analyzer = analyzer
        self.num_speakers = _int_arg(num_speakers, 1, MAX_SPEAKERS, who, "num_speakers")
        self.iterations = _int_arg(iterations, 1, cgmm.MAX_ITERS, who, "iterations")
        self.refine = _int_arg(refine, 1, MAX_REFINE, who, "refine")
        self.seed = _int_arg(seed, 0, 2 ** 63 - 1, who, "seed")
        self.diag_load = _diag_load_arg(diag_load, who)
        self.last_ll = self.last_cov = self.last_perm = self.last_margin = self.last_nonfinite = None

    def analyze(self, wav):
        """(C, n) CUDA float32 -> complex64 (C, N, F), without dither"""
        return beamform.analyze_channels(self.analyzer, wav, "CgmmSeparator", cgmm.MAX_CHANNELS)

    def masks(self, spec):
        m = cgmm.cgmm_masks(spec, self.num_speakers + 1, self.iterations, init="random", seed=self.seed,
                            diag_load=self.diag_load)
        self.last_ll, self.last_nonfinite = cgmm.last_ll, cgmm.last_nonfinite
        m, self.last_cov, _ = align_permutations(m, cgmm.last_cov, cgmm.last_log_alpha, self.refine)
        self.last_perm, self.last_margin = last_perm, last_margin
        return m


def separate(specs, masks, ref=0, diag_load=1e-3):
    """specs: complex64 (C, N, F); masks: float32 (K, N, F) with the speakers first and the noise last (CgmmSeparator.masks).
    Speaker s is beamformed with the covariance of mask s as the target and that of 1 - mask s as the interference (one
    covariance pass, one mvdr_weights call and one apply_weights call for the whole list of (utterance, speaker) pairs).
    Returns the K - 1 spectra (N, F) of an utterance as a list; for lists of utterances, a list of such lists."""
    who = "separate"
    sp, many, Cn, F, dev = _check_specs(specs, who, beamform.MAX_CHANNELS)
    if isinstance(masks, (list, tuple)) != many:
        raise ValueError("%s: specs and masks are both tensors or both lists" % who)
    ms, _, K, Fm, devm = _check_masks(masks, who)
    if len(ms) != len(sp) or Fm != F or devm != dev:
        raise ValueError("%s: %d spectra with %d bins on %s, %d masks with %d bins on %s"
                         % (who, len(sp), F, dev, len(ms), Fm, devm))
    for i, (s, m) in enumerate(zip(sp, ms)):
        if m.shape[1] != s.shape[1]:
            raise ValueError("%s: utterance %d: the masks have %d frames, the spectrum %d" % (who, i, m.shape[1], s.shape[1]))
    beamform._ref_arg(ref, Cn, who)
    diag_load = _diag_load_arg(diag_load, who)
    S = K - 1
    pairs_spec = [s for s in sp for _ in range(S)]
    phi = beamform.spatial_covariance(pairs_spec, [m[k] for m in ms for k in range(S)], complement=True)
    w, _ = beamform.mvdr_weights([p[0] for p in phi], [p[1] for p in phi], ref, diag_load)
    out = beamform.apply_weights(pairs_spec, w)
    out = [out[i * S:(i + 1) * S] for i in range(len(sp))]
    return out if many else out[0]
