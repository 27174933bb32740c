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
