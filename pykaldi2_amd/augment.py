"""Waveform augmentation on the device: sampling-rate conversion, speed and volume perturbation.

Kaldi's chain recipes perturb every utterance before anything else: `sox speed` by 0.9 / 1.0 / 1.1 (a resampling that changes
tempo and pitch) and a random volume.  Here the whole ragged minibatch is converted by one launch of the library's polyphase
windowed-sinc resampler (csrc/resample.hip: Kaldi's LinearResample restated); every utterance has its own
ratio, length and gain, and nothing returns to the host.

  ResamplePlan(rate_in, rate_out)           host object: taps and weights per output phase (needs no GPU)
  resample(x, rate_in, rate_out, gain)      (n,) or (R, n) CUDA float32
  resample_ragged(wav, lens, ratios, gains) the 1-D concatenation data.sequence_batches yields
  speed_perturb(wav, lens, factors, fs)     factor s = resample round(fs s) -> fs
  WaveAugment                               the per-utterance draws of data_config `speed_perturb` / `volume_perturb`

and feature augmentation, SpecAugment in interval form (csrc/spec_augment.hip): time warp, frequency and time
masks on the packed rows FbankExtractor returns, one launch per minibatch, in place when nothing warps.

  spec_augment(feats, row_off, frames, plan) a host plan (validated without a GPU) applied to the minibatch
  SpecAugment                               the per-utterance draws of data_config `spec_augment`
"""
import ctypes as C
import math
import sys

import numpy as np
import torch

from . import _lib

PATH_NONE, PATH_LDS, PATH_MEM = 0, 1, 2      # PK2_RESAMPLE_PATH_*: last_path() is their OR over the jobs of a launch
_PLANS = {}


class ResamplePlan:
    """pk2_resample_plan: one per (rate_in, rate_out, cutoff, num_zeros), kept for the life of the process (its device
    tables are uploaded by the first launch on a device)."""

    def __new__(cls, rate_in, rate_out, cutoff=None, num_zeros=6):
        key = (int(rate_in), int(rate_out), None if cutoff is None else float(cutoff), int(num_zeros))
        plan = _PLANS.get(key)
        if plan is None:
            plan = super().__new__(cls)
            plan._create(*key)
            _PLANS[key] = plan
        return plan

    def _create(self, rate_in, rate_out, cutoff, num_zeros):
        h = C.c_void_p()
        _lib.check(_lib.lib().pk2_resample_plan_create(rate_in, rate_out, 0.0 if cutoff is None else cutoff, num_zeros,
                                                       C.byref(h)))
        self.handle, self.rate_in, self.rate_out = h, rate_in, rate_out
        iu, ou, mt, tile, nbytes = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().pk2_resample_plan_info(h, C.byref(iu), C.byref(ou), C.byref(mt), C.byref(tile), C.byref(nbytes)))
        self.iu, self.ou, self.max_taps, self.tile, self.table_bytes = iu.value, ou.value, mt.value, tile.value, nbytes.value

    def num_output(self, n):
        out = _lib.lib().pk2_resample_num_output(self.handle, int(n))
        if out < 0:
            _lib.check(-1)
        return int(out)

    def export(self):
        """(first (ou) int32, taps (ou) int32, weights (ou, max_taps) float32, zero beyond taps[p])."""
        first, taps = np.zeros(self.ou, np.int32), np.zeros(self.ou, np.int32)
        w = np.zeros((self.ou, self.max_taps), np.float32)
        _lib.check(_lib.lib().pk2_resample_plan_export(self.handle, _lib.ptr(first), _lib.ptr(taps), _lib.ptr(w)))
        return first, taps, w


def last_path():
    p = C.c_int32(-1)
    _lib.check(_lib.lib().pk2_resample_last_path(C.byref(p)))
    return p.value


def _launch(jobs, device):
    """jobs: (plan, in tensor, out tensor, gain); ceil(len / RESAMPLE_MAX_JOBS) launches."""
    stream = _lib.stream_ptr(device)
    for b in range(0, len(jobs), _lib.RESAMPLE_MAX_JOBS):
        part = jobs[b:b + _lib.RESAMPLE_MAX_JOBS]
        tab = (_lib.ResampleJob * len(part))()
        for t, (plan, x, y, gain) in zip(tab, part):
            t.plan, t.inp, t.n_in, t.out, t.n_out, t.gain = plan.handle, x.data_ptr(), x.numel(), y.data_ptr(), y.numel(), gain
        _lib.check(_lib.lib().pk2_resample_batch(tab, len(part), stream))


def _check(x, what):
    _lib.require_gpu()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError("%s: expected a contiguous CUDA float32 tensor" % what)
    return x


def resample(x, rate_in, rate_out, gain=1.0):
    """x: (n,) or (R, n) CUDA float32 -> (n_out,) / (R, n_out), n_out = ceil(n rate_out / rate_in)."""
    _check(x, "resample")
    if x.dim() not in (1, 2) or x.numel() == 0:
        raise ValueError("resample: expected a non-empty (n,) or (R, n) tensor")
    plan = ResamplePlan(rate_in, rate_out)
    rows = x.view(-1, x.shape[-1])
    out = torch.empty(rows.shape[0], plan.num_output(rows.shape[1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _launch([(plan, r, o, float(gain)) for r, o in zip(rows, out)], x.device)
    return out.view(-1) if x.dim() == 1 else out


def resample_ragged(wav, lens, ratios, gains=None):
    """wav: 1-D CUDA float32, the utterances back to back; lens: their lengths; ratios: (rate_in, rate_out) per utterance;
    gains: a factor per utterance (None: 1).  Returns (new wav, new lens) in the same layout, made by one launch; a row
    with rate_in == rate_out is copied (times its gain).  When no row changes at all, `wav` itself comes back."""
    _check(wav, "resample_ragged")
    n = len(lens)
    gains = [1.0] * n if gains is None else [float(g) for g in gains]
    if wav.dim() != 1 or len(ratios) != n or len(gains) != n or sum(lens) != wav.numel() or min(lens, default=0) < 1:
        raise ValueError("resample_ragged: wav must be the 1-D concatenation of len(lens) non-empty rows, one ratio (and gain) each")
    if all(int(fi) == int(fo) for fi, fo in ratios) and all(g == 1.0 for g in gains):
        return wav, list(lens)
    plans = [ResamplePlan(fi, fo) for fi, fo in ratios]
    new_lens = [p.num_output(m) for p, m in zip(plans, lens)]
    out = torch.empty(sum(new_lens), dtype=torch.float32, device=wav.device)
    jobs, a, b = [], 0, 0
    for p, m, k, g in zip(plans, lens, new_lens, gains):
        jobs.append((p, wav[a:a + m], out[b:b + k], g))
        a, b = a + m, b + k
    with torch.cuda.device(wav.device):
        _launch(jobs, wav.device)
    return out, new_lens


def speed_ratio(factor, fs=16000):
    """Speed perturbation by `factor` at sampling rate fs = resampling round(fs factor) -> fs (`sox speed`)."""
    return int(round(fs * float(factor))), int(fs)


def speed_perturb(wav, lens, factors, fs=16000, gains=None):
    return resample_ragged(wav, lens, [speed_ratio(s, fs) for s in factors], gains)


class WaveAugment:
    """Per-utterance speed factor (drawn uniformly from `speed_factors`) and volume gain (uniform in `volume_range`).  The
    draws come from a generator of their own, np.random.default_rng([seed, rank, epoch, 104729]): numpy's global stream, which
    the dynamic simulation draws from, is never touched."""

    def __init__(self, speed_factors=None, volume_range=None, seed=0, fs=16000):
        if speed_factors is not None:
            if isinstance(speed_factors, (str, bytes)) or not hasattr(speed_factors, "__len__"):
                raise ValueError("speed_perturb: expected a list of factors")
            speed_factors = [float(s) for s in speed_factors]
            if not speed_factors:
                raise ValueError("speed_perturb: the list of factors is empty")
            if any(not (0.5 <= s <= 2.0) for s in speed_factors):
                raise ValueError("speed_perturb: factors must lie in [0.5, 2.0], got %r" % (speed_factors,))
        if volume_range is not None:
            if isinstance(volume_range, (str, bytes)) or not hasattr(volume_range, "__len__") or len(volume_range) != 2:
                raise ValueError("volume_perturb: expected [low, high]")
            volume_range = (float(volume_range[0]), float(volume_range[1]))
            if not (math.isfinite(volume_range[0]) and math.isfinite(volume_range[1])) or volume_range[0] > volume_range[1]:
                raise ValueError("volume_perturb: low > high in %r" % (volume_range,))
        self.speed_factors, self.volume_range, self.seed, self.fs = speed_factors, volume_range, int(seed), int(fs)

    @classmethod
    def from_config(cls, config, seed=0):
        """data_config `speed_perturb`: [factor, ...]; `volume_perturb`: [low, high].  None when neither is present."""
        dc = config.get("data_config") or {}
        if dc.get("speed_perturb") is None and dc.get("volume_perturb") is None:
            return None
        return cls(dc.get("speed_perturb"), dc.get("volume_perturb"), seed)

    def changes_length(self):
        return self.speed_factors is not None and any(s != 1.0 for s in self.speed_factors)

    def generator(self, rank=0, epoch=0):
        return np.random.default_rng([self.seed, int(rank), int(epoch), 104729])

    def draw(self, gen, n):
        """(speed factors, gains) of the next n utterances from `gen` (self.generator(rank, epoch))."""
        factors = [1.0] * n
        gains = [1.0] * n
        if self.speed_factors is not None:
            factors = [self.speed_factors[int(i)] for i in gen.integers(len(self.speed_factors), size=n)]
        if self.volume_range is not None:
            gains = [float(g) for g in gen.uniform(self.volume_range[0], self.volume_range[1], size=n)]
        return factors, gains

    def ratios(self, factors):
        return [speed_ratio(s, self.fs) for s in factors]


def refuse_speed_perturb(config, prog):
    """For the trainers that read frame-level labels (made for the unperturbed length): exit with a one-line message when
    data_config `speed_perturb` holds a factor other than 1."""
    sp = (config.get("data_config") or {}).get("speed_perturb")
    aug = WaveAugment(sp) if sp is not None else None
    if aug is not None and aug.changes_length():
        sys.stderr.write("ERROR: %s reads frame-level labels and cannot train on speed-perturbed audio: remove data_config "
                         "speed_perturb %r (bin/train_chain.py -e2e honours it)\n" % (prog, sp))
        sys.exit(2)


NUM_BINS = 80
SPEC_KEYS = ("freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "time_warp", "fill")
_SPEC_FREQ0, _SPEC_TIME0 = 2, 2 + 2 * _lib.SPEC_MAX_FREQ_MASKS      # plan row: c, d, frequency pairs, time pairs


def _check_plan(plan, frames):
    """The host plan of pk2_spec_augment against the frame counts: ValueError, or whether any row warps.  Needs no GPU."""
    if not (isinstance(plan, np.ndarray) and plan.dtype == np.int32 and plan.ndim == 2 and plan.flags.c_contiguous
            and plan.shape == (len(frames), _lib.SPEC_PLAN_STRIDE) and len(frames) >= 1):
        raise ValueError("spec_augment: the plan must be a host int32 array [%d, %d], one row per utterance"
                         % (len(frames), _lib.SPEC_PLAN_STRIDE))
    T = np.asarray(frames, dtype=np.int64).reshape(-1, 1)
    if T.min() < 1:
        raise ValueError("spec_augment: every utterance needs at least one frame")
    p = plan.astype(np.int64)
    for what, lo, hi, limit in (("frequency", _SPEC_FREQ0, _SPEC_TIME0, NUM_BINS), ("time", _SPEC_TIME0, plan.shape[1], T)):
        a, b = p[:, lo:hi:2], p[:, lo + 1:hi:2]
        bad = np.argwhere((a < 0) | (a > b) | (b > limit))
        if len(bad):
            n, k = (int(v) for v in bad[0])
            raise ValueError("spec_augment: utterance %d (%d frames): %s interval [%d, %d) outside 0 <= a <= b <= %d"
                             % (n, int(T[n, 0]), what, a[n, k], b[n, k], NUM_BINS if what == "frequency" else int(T[n, 0])))
    c, d = p[:, 0:1], p[:, 1:2]
    warps = c != d
    bad = np.argwhere(warps & ((c < 1) | (d < 1) | (c > T - 2) | (d > T - 2)))
    if len(bad):
        n = int(bad[0][0])
        raise ValueError("spec_augment: utterance %d (%d frames): warp (c, d) = (%d, %d) needs c == d or 1 <= c, d <= T - 2"
                         % (n, int(T[n, 0]), c[n, 0], d[n, 0]))
    return bool(warps.any())


def spec_augment(feats, row_off, frames, plan, fill=0.0, out=None):
    """pk2_spec_augment on feats [sum(frames), 80] (what FbankExtractor.__call__ returns, with its row_off): time warp, then
    the frequency and time masks of the host `plan` (int32 [N, SPEC_PLAN_STRIDE], SpecAugment.draw), in one launch.  The plan
    is validated against `frames` before anything touches the GPU.  out=None: in place when no row warps (only the masked
    elements are written), else a new tensor; `out is feats` with a warping plan raises ValueError.  Returns the result."""
    has_warp = _check_plan(plan, frames)
    if not math.isfinite(float(fill)):
        raise ValueError("spec_augment: fill must be finite, got %r" % (fill,))
    if out is feats and out is not None and has_warp:
        raise ValueError("spec_augment: a warping plan cannot run in place (out is feats)")
    _check(feats, "spec_augment")
    total = int(sum(int(t) for t in frames))
    if feats.dim() != 2 or tuple(feats.shape) != (total, NUM_BINS):
        raise ValueError("spec_augment: expected feats [%d, %d], got %r" % (total, NUM_BINS, tuple(feats.shape)))
    if not (isinstance(row_off, torch.Tensor) and row_off.device == feats.device and row_off.dtype == torch.int64
            and row_off.is_contiguous() and row_off.numel() == len(frames) + 1):
        raise ValueError("spec_augment: row_off must be the int64 [N + 1] tensor of FbankExtractor.__call__ on the device of feats")
    if out is None:
        out = torch.empty_like(feats) if has_warp else feats
    elif out is not feats:
        _check(out, "spec_augment")
        if out.shape != feats.shape or out.device != feats.device:
            raise ValueError("spec_augment: out must have the shape and device of feats")
    with torch.cuda.device(feats.device):
        plan_dev = _lib.h2d(plan, feats.device)
        _lib.check(_lib.lib().pk2_spec_augment(_lib.ptr(feats), _lib.ptr(out), _lib.ptr(row_off), len(frames), total,
                                               _lib.ptr(plan_dev), 1 if has_warp else 0, float(fill),
                                               _lib.stream_ptr(feats.device)))
    return out


class SpecAugment:
    """SpecAugment (Park et al. 2019) in interval form, data_config `spec_augment`: per utterance of T frames an optional
    time warp (`time_warp` = W > 0 and T >= 2 W + 3: centre c uniform in [W + 1, T - W - 2] moves to c + w, w uniform in
    [-W, W]), `freq_masks` bin intervals of width uniform in [0, freq_width], and `time_masks` frame intervals of width
    uniform in [0, min(time_width, floor(time_ratio T))]; masked elements become `fill` (0 is the utterance mean after CMN or
    -transform).  The draws come from a generator of their own, np.random.default_rng([seed, rank, epoch, 611953]): numpy's
    global stream and WaveAugment's draws are never touched."""

    def __init__(self, freq_masks=2, freq_width=27, time_masks=2, time_width=40, time_ratio=0.2, time_warp=0, fill=0.0, seed=0):
        def integer(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError("spec_augment: %s must be an integer %s, got %r"
                                 % (name, ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi), v))
            return int(v)
        self.freq_masks = integer("freq_masks", freq_masks, 0, _lib.SPEC_MAX_FREQ_MASKS)
        self.freq_width = integer("freq_width", freq_width, 0, NUM_BINS)
        self.time_masks = integer("time_masks", time_masks, 0, _lib.SPEC_MAX_TIME_MASKS)
        self.time_width = integer("time_width", time_width, 0, None)
        self.time_warp = integer("time_warp", time_warp, 0, None)
        if isinstance(time_ratio, bool) or not isinstance(time_ratio, (int, float, np.integer, np.floating)) \
                or not (0.0 <= float(time_ratio) <= 1.0):
            raise ValueError("spec_augment: time_ratio must lie in [0, 1], got %r" % (time_ratio,))
        if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)) or not math.isfinite(float(fill)):
            raise ValueError("spec_augment: fill must be a finite number, got %r" % (fill,))
        self.time_ratio, self.fill, self.seed = float(time_ratio), float(fill), int(seed)

    @classmethod
    def from_config(cls, config, seed=0):
        """data_config `spec_augment`: true (the defaults) or a mapping over them (a key it does not know raises KeyError);
        None when the key is absent or false."""
        sa = (config.get("data_config") or {}).get("spec_augment")
        if sa is None or sa is False:
            return None
        if sa is True:
            return cls(seed=seed)
        if not isinstance(sa, dict):
            raise ValueError("spec_augment: expected true or a mapping, got %r" % (sa,))
        for k in sa:
            if k not in SPEC_KEYS:
                raise KeyError("spec_augment: unknown key %r (known: %s)" % (k, ", ".join(SPEC_KEYS)))
        return cls(seed=seed, **sa)

    def generator(self, rank=0, epoch=0):
        return np.random.default_rng([self.seed, int(rank), int(epoch), 611953])

    def draw(self, gen, frames):
        """The host plan (int32 [N, SPEC_PLAN_STRIDE]) of the next utterances from `gen` (self.generator(rank, epoch))."""
        plan = np.zeros((len(frames), _lib.SPEC_PLAN_STRIDE), np.int32)
        W = self.time_warp
        for row, T in zip(plan, frames):
            T = int(T)
            if W > 0 and T >= 2 * W + 3:
                c = int(gen.integers(W + 1, T - W - 1))          # uniform in [W + 1, T - W - 2]
                row[0], row[1] = c, c + int(gen.integers(-W, W + 1))
            for k in range(self.freq_masks):
                width = int(gen.integers(0, self.freq_width + 1))
                a = int(gen.integers(0, NUM_BINS - width + 1))
                row[_SPEC_FREQ0 + 2 * k], row[_SPEC_FREQ0 + 2 * k + 1] = a, a + width
            widest = min(self.time_width, int(math.floor(self.time_ratio * T)))
            for k in range(self.time_masks):
                width = int(gen.integers(0, widest + 1))
                a = int(gen.integers(0, T - width + 1))
                row[_SPEC_TIME0 + 2 * k], row[_SPEC_TIME0 + 2 * k + 1] = a, a + width
        return plan

    def __call__(self, feats, row_off, frames, gen, out=None):
        return spec_augment(feats, row_off, frames, self.draw(gen, frames), self.fill, out)

    def epoch(self, rank=0, epoch=0):
        """The callable (feats, row_off, frames, out=None) -> feats of one training epoch: the `spec` argument of the
        se.sequence_loss* functions and the call the trainers make after `transform(feats)`."""
        gen = self.generator(rank, epoch)
        return lambda feats, row_off, frames, out=None: self(feats, row_off, frames, gen, out)


def refuse_time_warp(config, prog):
    """For the trainers that read frame-level labels: a time warp moves frames under the labels, so exit with a one-line
    message when data_config `spec_augment` has time_warp > 0.  The masks are honoured everywhere."""
    aug = SpecAugment.from_config(config)
    if aug is not None and aug.time_warp > 0:
        sys.stderr.write("ERROR: %s reads frame-level labels and cannot train on time-warped features: set data_config "
                         "spec_augment time_warp %r to 0 (bin/train_chain.py -e2e honours it)\n" % (prog, aug.time_warp))
        sys.exit(2)
