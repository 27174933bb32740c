"""Dynamic data simulation on the device: reverberation by a room impulse response and additive noise at a
sampled SNR, the single-channel / single-source path of the reference's simulator (reference
simulation/simulation.py:181-234 `SimpleSimulator`, simulation/_distorter.py:84-154 `Distorter`), which the
reference runs with numpy inside DataLoader workers (data/sr_dataset.py:321-345).  Waveforms, impulse responses
and noises are CUDA float32 tensors; the power / peak statistics stay in device memory between the kernels of an
utterance (no host round trip), only the random draws are made on the host -- with numpy's global generator and
in the reference's order, so `np.random.seed` reproduces the reference's choices.

Multi-channel / multi-source simulation (reference `_Simulator.simulate` with a `Mixer`, `MultiSourceSimulator`,
`generate_isotropic_noise`): the DEVICE LAYOUT IS CHANNEL-MAJOR -- a multi-channel signal is a contiguous CUDA float32
(C, T) tensor and a multi-channel RIR is (C, k), as `rirgen.xp_rirgen` returns them per source; the reference uses
(T, C).  Scales, powers, peaks and delays stay in device memory; the draws (SPR, start samples, SNRs) are made on the
host in the reference's order.

Reference behaviours kept on purpose (oracle/simulation_ref.py): the SNR of a directional noise comes from
uniform[0, 20] dB whatever `snr_range` is; the power used to scale a second noise already includes the first.
"""
import functools

import numpy as np
import torch

from . import _lib


def _check(x):
    _lib.require_gpu()
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous(), "expected a 1-D CUDA float32 tensor"
    return x


def _power(x):
    """device f64[2] = (sum of squares, max |x|)"""
    stats = torch.zeros(2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().pk2_sim_power(_lib.ptr(x), x.numel(), _lib.ptr(stats), _lib.stream_ptr(x.device)))
    return stats


class Distorter:
    """Distorter.apply_rir / Distorter.add_noise of the reference on CUDA tensors."""

    @staticmethod
    def apply_rir(wav, rir, delay=None, get_early_reverb=False, fs=16000):
        """1-D `rir`: reverberant signal, sample-synchronised with the input (sync=True): (rir * wav)[delay-1 : delay+n-1] with
        delay = argmax(rir).  `delay` may be passed when it is known (it costs a host read otherwise): an int, or a
        one-element CUDA int32 tensor that the kernel reads in device memory (the argmax that rirgen writes).

        2-D `rir` (C, k), channel-major: returns the (C, n) reverberant signal, every channel shifted by the delay of
        channel 0 (the reference's int(np.argmax(rir, axis=0)[0])); `delay` may be an int or a CUDA int32 tensor whose
        first element is that delay (a row of rirgen's `delays`).  get_early_reverb=True returns (reverb, early_reverb),
        early_reverb = the convolution with the taps [0, min(k, int(0.04 fs + delay))) only."""
        if rir.dim() == 2 or get_early_reverb:
            one_d = rir.dim() == 1
            rv, er = _apply_rir_batch([wav], [rir.view(1, -1) if one_d else rir], [delay], get_early_reverb, fs)
            rv, er = (rv[0].view(-1), er[0].view(-1) if er[0] is not None else None) if one_d else (rv[0], er[0])
            return (rv, er) if get_early_reverb else rv
        wav, rir = _check(wav), _check(rir)
        if isinstance(delay, torch.Tensor):
            assert delay.is_cuda and delay.dtype == torch.int32 and delay.numel() == 1, "expected a CUDA int32 delay"
            delay = delay.reshape(1)
            out = torch.empty_like(wav)
            _lib.check(_lib.lib().pk2_sim_apply_rir_dev(_lib.ptr(wav), wav.numel(), _lib.ptr(rir), rir.numel(),
                                                        _lib.ptr(delay), _lib.ptr(out), _lib.stream_ptr(wav.device)))
            return out
        if delay is None:
            delay = int(torch.argmax(rir).item())
        out = torch.empty_like(wav)
        _lib.check(_lib.lib().pk2_sim_apply_rir(_lib.ptr(wav), wav.numel(), _lib.ptr(rir), rir.numel(), int(delay),
                                                _lib.ptr(out), _lib.stream_ptr(wav.device)))
        return out

    @staticmethod
    def add_noise(signal, noise, snr, start=None, noise_position_scheme='sample_noise'):
        """signal + noise scaled to `snr` dB and placed by the 'sample_noise' scheme.  `start` = the sampled position
        (drawn here like the reference does when None).  Returns (distorted, start); `signal` is not modified.

        2-D inputs are (C, n) and (C, m), channel-major; the powers are means over all channels.
        noise_position_scheme='repeat_noise': a shorter noise is tiled ceil(n / m) times, then n samples are taken from
        `start`, drawn as np.random.randint(0, high=n_sample - n) (no draw when the lengths are equal after tiling)."""
        if noise_position_scheme not in ('sample_noise', 'repeat_noise'):
            raise ValueError("Unknown noise position scheme %s" % (noise_position_scheme,))
        if signal.dim() == 2 or noise.dim() == 2 or noise_position_scheme == 'repeat_noise':
            one_d = signal.dim() == 1
            sig2 = _check_mc(signal.view(1, -1) if one_d else signal, "signal")
            nz2 = _check_mc(noise.view(1, -1) if noise.dim() == 1 else noise, "noise")
            out = sig2.clone()
            start = _add_noise_mc(out, nz2, snr, start, noise_position_scheme == 'repeat_noise')
            return (out.view(-1) if one_d else out), start
        signal, noise = _check(signal), _check(noise)
        n, m = signal.numel(), noise.numel()
        if start is None:
            n_extra = abs(n - m)
            start = int(np.random.randint(0, high=n_extra, size=1)[0]) if n_extra > 0 else 0     # _sampling.get_sample 'uniform_int'
        out = signal.clone()
        ps, pn = _power(signal), _power(noise)       # both alive until the kernel that reads them is enqueued
        _lib.check(_lib.lib().pk2_sim_add_noise(_lib.ptr(out), n, _lib.ptr(noise), m, int(start), float(snr),
                                                _lib.ptr(ps), _lib.ptr(pn), _lib.stream_ptr(signal.device)))
        return out, start


class SimpleSimulator:
    """Single speech source simulator (reference simulation/simulation.py:181-234):
    ``SimpleSimulator(use_rir, use_noise, snr_range)(source_wav, dir_noise_wavs, source_rir, dir_noise_rirs,
    normalize_gain=...)`` -> (simulated waveform, sentence config).  A 2-D `source_rir` (C, k) (and (C, k') noise
    RIRs) takes the multi-channel path and returns the (C, T) mixture.  gen_mask=True returns the reference's 4-tuple
    (mixed, [early reverberation], [mask (N, F)], sentence config), computed by the `mask_estimator` the simulator was
    built with (see MultiSourceSimulator); `mask_seed` seeds the analyzer's dither."""

    def __init__(self, array_geometry=None, use_rir=True, use_noise=True, snr_range=(0, 30), mask_estimator=None):
        self.array_geometry = array_geometry        # not read: the channels come from the RIRs (as in the reference)
        self.use_rir, self.use_noise = use_rir, use_noise
        self.snr_range = tuple(snr_range)      # sets `global_snr` in the reference, which its simulate() never reads
        self.mask_estimator = mask_estimator   # what gen_mask=True computes the masks with

    def __call__(self, source_wav, dir_noise_wavs=None, source_rir=None, dir_noise_rirs=None, normalize_gain=True,
                 rir_delays=None, gen_mask=False, mask_seed=None):
        if gen_mask:
            _require_mask_estimator(self.mask_estimator)
            # the reference's 4-tuple (mixed, [early reverberation], [mask], sent_cfg); 1-D inputs come back 1-D
            one_d = source_wav.dim() == 1 and (source_rir is None or source_rir.dim() == 1)
            mixed, early, cfg = _simulate([source_wav], dir_noise_wavs, [source_rir] if source_rir is not None else None,
                                          dir_noise_rirs, None, normalize_gain, True, rir_delays, None,
                                          mask_estimator=self.mask_estimator, mask_seed=mask_seed)
            mask = cfg.pop('mask')
            if one_d:
                mixed, early = mixed.view(-1), [e.view(-1) for e in early]
            return mixed, early, mask, cfg
        if source_rir is not None and source_rir.dim() == 2:
            mixed, _, cfg = _simulate([source_wav], dir_noise_wavs, [source_rir], dir_noise_rirs, None, normalize_gain, False,
                                      rir_delays, None)
            return mixed, cfg
        noises = list(dir_noise_wavs) if dir_noise_wavs is not None else []
        use_rir = source_rir is not None
        if use_rir and noises:
            assert dir_noise_rirs is not None and len(dir_noise_rirs) == len(noises), \
                "number of dir_noise_rir does not equal to number of directional noise sources"
        delays = list(rir_delays) if rir_delays is not None else [None] * (1 + len(noises))
        mixed = Distorter.apply_rir(source_wav, source_rir, delays[0]) if use_rir else _check(source_wav).clone()
        cfg = {}
        if noises:
            cfg["dir_snr"] = np.random.uniform(low=0.0, high=20.0, size=len(noises))      # config.py:39-40
            cfg["dir_start"] = []
            stream = _lib.stream_ptr(mixed.device)
            for i, nz in enumerate(noises):
                nz = Distorter.apply_rir(nz, dir_noise_rirs[i], delays[1 + i]) if use_rir else _check(nz)
                n, m = mixed.numel(), nz.numel()
                n_extra = abs(n - m)
                start = int(np.random.randint(0, high=n_extra, size=1)[0]) if n_extra > 0 else 0
                cfg["dir_start"].append(start)
                ps, pn = _power(mixed), _power(nz)
                _lib.check(_lib.lib().pk2_sim_add_noise(_lib.ptr(mixed), n, _lib.ptr(nz), m, start, float(cfg["dir_snr"][i]),
                                                        _lib.ptr(ps), _lib.ptr(pn), stream))
        if normalize_gain:
            peak = _power(mixed)
            _lib.check(_lib.lib().pk2_sim_gain_norm(_lib.ptr(mixed), mixed.numel(), _lib.ptr(peak),
                                                    _lib.stream_ptr(mixed.device)))
        return mixed, cfg


# ---------------------------------------------------------------------------------------------------------------------
# multi-channel / multi-source path: channel-major (C, T) CUDA float32 tensors
# ---------------------------------------------------------------------------------------------------------------------
def _check_mc(x, what="signal"):
    _lib.require_gpu()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
            and x.numel() > 0):
        raise ValueError("%s: expected a contiguous 2-D (channels, samples) CUDA float32 tensor" % what)
    return x


def _stats(n=1, device=None):
    return torch.zeros(n, 2, dtype=torch.float64, device=device)


def _apply_rir_batch(wavs, rirs, delays, get_early_reverb=False, fs=16000):
    """All (source, channel) rows in one launch.  wavs[i] (n_i,), rirs[i] (C, k_i), delays[i] None | int | CUDA int32 tensor
    (its first element: the delay of channel 0).  Returns ([reverb (C, n_i)], [early (C, n_i) | None])."""
    if len(wavs) != len(rirs):
        raise ValueError("number of RIRs (%d) does not equal to number of sources (%d)" % (len(rirs), len(wavs)))
    delays = list(delays) if delays is not None else [None] * len(wavs)
    if len(delays) != len(wavs):
        raise ValueError("number of delays (%d) does not equal to number of sources (%d)" % (len(delays), len(wavs)))
    jobs, keep, reverb, early = [], [], [], []
    C = None
    for i, (wav, rir) in enumerate(zip(wavs, rirs)):
        wav = _check(wav)
        rir = _check_mc(rir.view(1, -1) if rir.dim() == 1 else rir, "rir")
        if C is None:
            C = rir.shape[0]
        if rir.shape[0] != C:
            raise ValueError("RIR %d has %d channels, the first one %d" % (i, rir.shape[0], C))
        n, k = wav.numel(), rir.shape[1]
        out = torch.empty(C, n, dtype=torch.float32, device=wav.device)
        er = torch.empty_like(out) if get_early_reverb else None
        d, d_dev = delays[i], None
        if isinstance(d, torch.Tensor):
            if not (d.is_cuda and d.dtype == torch.int32 and d.numel() >= 1):
                raise ValueError("expected a CUDA int32 delay")
            d_dev, d = d.reshape(-1), 0
        elif d is None:
            d = int(torch.argmax(rir[0]).item())
        jobs.append(_lib.SimRirJob(wav.data_ptr(), rir.data_ptr(), out.data_ptr(), er.data_ptr() if er is not None else None,
                                   d_dev.data_ptr() if d_dev is not None else None, n, k, int(d)))
        keep.append((wav, rir, d_dev))
        reverb.append(out)
        early.append(er)
    stream = _lib.stream_ptr(reverb[0].device)
    for j0 in range(0, len(jobs), _lib.SIM_MAX_SEGS):
        chunk = jobs[j0:j0 + _lib.SIM_MAX_SEGS]
        _lib.check(_lib.lib().pk2_sim_apply_rir_mc((_lib.SimRirJob * len(chunk))(*chunk), len(chunk), C, int(0.04 * fs), stream))
    return reverb, early


def _power_seg(tensors):
    """device f64 (len, 2): (sum of squares, max |x|) of every tensor over all its channels, one launch"""
    if len(tensors) > _lib.SIM_MAX_SEGS:
        raise ValueError("at most %d signals per call" % _lib.SIM_MAX_SEGS)
    stats = _stats(len(tensors), tensors[0].device)
    segs = (_lib.SimSeg * len(tensors))(*[_lib.SimSeg(t.data_ptr(), t.numel()) for t in tensors])
    _lib.check(_lib.lib().pk2_sim_power_seg(segs, len(tensors), _lib.ptr(stats), _lib.stream_ptr(tensors[0].device)))
    return stats


def _add_noise_mc(mixed, noise, snr, start, repeat):
    """mixed (C, n) += noise (C, m) at `snr` dB, in place; returns the start (drawn like the reference when None)."""
    if mixed.shape[0] != noise.shape[0]:
        raise ValueError("noise has %d channels, the signal %d" % (noise.shape[0], mixed.shape[0]))
    C, n, m = mixed.shape[0], mixed.shape[1], noise.shape[1]
    if start is None:
        if repeat:                                          # _NoiseSampler.repeat_noise
            n_sample = -(-n // m) * m if m < n else m
            start = 0 if n_sample == n else int(np.random.randint(0, high=n_sample - n, size=1)[0])
        else:                                               # _NoiseSampler.sample_noise
            n_extra = abs(n - m)
            start = int(np.random.randint(0, high=n_extra, size=1)[0]) if n_extra > 0 else 0
    st = _power_seg([mixed, noise])
    _lib.check(_lib.lib().pk2_sim_add_noise_mc(_lib.ptr(mixed), n, _lib.ptr(noise), m, C, int(start), float(snr), int(repeat),
                                               _lib.ptr(st[0]), _lib.ptr(st[1]), _lib.stream_ptr(mixed.device)))
    return int(start)


class MixerConfig:
    """Configurations on mixing speech sources (reference simulation/_mixer.py:5-19)."""

    def __init__(self, spr_range=(-2.5, 2.5)):
        self.config = dict()
        self.config['mixed_length'] = {'scheme': 'longest_source', 'min': 5}
        self.config['positioning'] = {'scheme': 'random_start'}
        self.config['ref_source'] = 'first_source'
        self.config['spr'] = {'min': float(spr_range[0]), 'max': float(spr_range[1]), 'distribution': 'uniform'}


class Mixer:
    """Mixes speech signals to simulate overlapping speech (reference simulation/_mixer.py:22-107) on (C, n_i) CUDA
    tensors, channel-major."""

    def __init__(self, config=None):
        config = MixerConfig() if config is None else config
        self.config = config.config if isinstance(config, MixerConfig) else config

    def mix_signals(self, signals, spr=None, signal2=None, want_positioned=True):
        """signals: list of (C, n_i) CUDA float32 tensors; spr: the n - 1 signal power ratios in dB against source 0
        (drawn from uniform[spr range] when None); signal2: a second list scaled and shifted like `signals` (the early
        reverberation).  Sources shorter than the longest get a start sample drawn from uniform_int[0, n_extra).
        Returns the reference's tuple (mixed (C, T), positioned_source, start_sample_idx, scale[, positioned_source2]):
        `scale` is a CUDA float64 (n, 1) tensor -- sqrt(P_0 / P_i 10^(spr_i / 10)), powers = means over the whole
        unpositioned source, computed on the device; positioned_source is None with want_positioned=False."""
        if self.config['mixed_length']['scheme'] != 'longest_source':
            raise ValueError("Mixer::mix_signals: Unknown mixed length scheme %s" % (self.config['mixed_length']['scheme']))
        if self.config['positioning']['scheme'] != 'random_start':
            raise ValueError("Mixer::mix_signals: Unknown mixing scheme %s" % (self.config['positioning']['scheme']))
        if self.config['ref_source'] != 'first_source':
            raise ValueError("Mixer::mix_signals: Unknown reference source %s" % (self.config['ref_source']))
        signals = [_check_mc(x, "signal %d" % i) for i, x in enumerate(signals)]
        nsrc, C = len(signals), signals[0].shape[0]
        if not 1 <= nsrc <= _lib.SIM_MAX_SEGS:
            raise ValueError("1 to %d sources per mixture" % _lib.SIM_MAX_SEGS)
        if any(x.shape[0] != C for x in signals):
            raise ValueError("the sources differ in their number of channels")
        if signal2 is not None:
            signal2 = [_check_mc(x, "signal2 %d" % i) for i, x in enumerate(signal2)]
            if len(signal2) != nsrc or any(a.shape != b.shape for a, b in zip(signals, signal2)):
                raise ValueError("signal2 does not correspond one-to-one with signals")
        T = max(x.shape[1] for x in signals)
        if spr is None:
            spr = np.random.uniform(low=float(self.config['spr']['min']), high=float(self.config['spr']['max']), size=nsrc - 1)
        spr = np.insert(np.asarray(spr, dtype=np.float64).reshape(-1), 0, 0)
        if spr.shape[0] != nsrc:
            raise ValueError("%d SPR values for %d sources" % (spr.shape[0] - 1, nsrc))
        starts = []
        for x in signals:                                   # _mix_by_random_start
            n_extra = T - x.shape[1]
            starts.append(int(np.random.randint(0, high=n_extra, size=1)[0]) if n_extra > 0 else 0)
        dev = signals[0].device
        stats = _power_seg(signals)
        mixed = torch.empty(C, T, dtype=torch.float32, device=dev)
        scale = torch.empty(nsrc, 1, dtype=torch.float64, device=dev)
        pos, pos2, tab = [], [], []
        for i, x in enumerate(signals):
            full = x.shape[1] == T
            p = (x if full else torch.empty(C, T, dtype=torch.float32, device=dev)) if want_positioned else None
            p2 = torch.empty(C, T, dtype=torch.float32, device=dev) if signal2 is not None else None
            pos.append(p)
            pos2.append(p2)
            tab.append(_lib.SimMixSrc(x.data_ptr(), signal2[i].data_ptr() if signal2 is not None else None,
                                      p.data_ptr() if p is not None and not full else None,
                                      p2.data_ptr() if p2 is not None else None, x.shape[1], starts[i], float(spr[i])))
        _lib.check(_lib.lib().pk2_sim_mix((_lib.SimMixSrc * nsrc)(*tab), nsrc, C, T, _lib.ptr(stats), _lib.ptr(mixed),
                                          _lib.ptr(scale), _lib.stream_ptr(dev)))
        ret = (mixed, pos if want_positioned else None, starts, scale)
        return ret + (pos2,) if signal2 is not None else ret


def _as_mc(x):
    return x.view(1, -1) if x.dim() == 1 else x


def _require_mask_estimator(est):
    if est is None:
        raise NotImplementedError("gen_mask: this simulator was built without a mask estimator; pass "
                                  "mask_estimator=MaskEstimator(SpectrumAnalyzer(...)) to its constructor")


def _simulate(source_wavs, dir_noise_wavs, source_rirs, dir_noise_rirs, iso_noise_wav, normalize_gain, get_early_reverb,
              rir_delays, mixer, fs=16000, mask_estimator=None, mask_seed=None):
    """_Simulator.simulate (reference simulation/simulation.py:55-178) as its text means it (the reference itself stops at
    the undefined `simu_cfg` with more than one source or an isotropic noise).  Draws, in its textual order: spr, the
    mixer's starts, dir_snr, each noise's start, iso_snr, the repeat-noise start.  `mixed_noisy` aliases `mixed` there, so
    every noise -- the isotropic one included -- is scaled against a power that contains the noises added before it.
    With a mask_estimator: the reference's step 5, cfg['mask'] = the list of the sources'
    masks -- channel 0 of every positioned early-reverberation signal against channel 0 of the noisy mixture, before the
    gain normalisation and after every other draw."""
    sources = list(source_wavs)
    noises = list(dir_noise_wavs) if dir_noise_wavs is not None else []
    n_source, n_noise = len(sources), len(noises)
    if n_source < 1:
        raise ValueError("no speech source")
    use_rir = source_rirs is not None and len(source_rirs) > 0
    cfg = {}
    if use_rir:
        if len(source_rirs) != n_source:
            raise ValueError('number of source_rir ({}) does not equal to number of source ({})'.format(len(source_rirs), n_source))
        if n_noise and (dir_noise_rirs is None or len(dir_noise_rirs) != n_noise):
            raise ValueError('number of dir_noise_rir does not equal to number of directional noise sources')
        delays = list(rir_delays) if rir_delays is not None else [None] * (n_source + n_noise)
        if len(delays) != n_source + n_noise:
            raise ValueError("rir_delays: one entry per source and per directional noise")
        reverb, early = _apply_rir_batch(sources, list(source_rirs), delays[:n_source], get_early_reverb, fs)
        noise_rv = _apply_rir_batch(noises, list(dir_noise_rirs), delays[n_source:], False, fs)[0] if n_noise else []
    else:
        reverb = [_check_mc(_as_mc(x), "source") for x in sources]
        early = [x.clone() for x in reverb] if get_early_reverb else [None] * n_source
        noise_rv = [_check_mc(_as_mc(x), "noise") for x in noises]
    if n_source == 1:
        mixed = reverb[0] if use_rir else reverb[0].clone()
        pos_early = early if get_early_reverb else None
    else:
        cfg['spr'] = np.random.uniform(low=float(mixer.config['spr']['min']), high=float(mixer.config['spr']['max']),
                                       size=n_source - 1)
        got = mixer.mix_signals(reverb, cfg['spr'], signal2=early if get_early_reverb else None, want_positioned=False)
        mixed, cfg['start_sample_idx'], cfg['scale'] = got[0], got[2], got[3]
        pos_early = got[4] if get_early_reverb else None
    if n_noise:
        cfg['dir_snr'] = np.random.uniform(low=0.0, high=20.0, size=n_noise)          # config.py:39-40
        cfg['dir_start'] = [_add_noise_mc(mixed, nz, cfg['dir_snr'][i], None, False) for i, nz in enumerate(noise_rv)]
    if iso_noise_wav is not None:
        cfg['iso_snr'] = np.random.uniform(low=10.0, high=30.0, size=1)               # ISONoiseConfig 'snr'
        cfg['iso_start'] = _add_noise_mc(mixed, _check_mc(_as_mc(iso_noise_wav), "iso_noise_wav"), cfg['iso_snr'][0], None, True)
    if mask_estimator is not None:
        cfg['mask'] = list(mask_estimator.get_mask_from_parallel_data([e[0] for e in pos_early], mixed[0], seed=mask_seed).unbind(0))
    if normalize_gain:
        bufs = [mixed] + (list(pos_early) if pos_early is not None else [])
        peak = _power_seg([mixed])
        gain = torch.empty(1, dtype=torch.float64, device=mixed.device)
        for j0 in range(0, len(bufs), _lib.SIM_MAX_SEGS):
            chunk = bufs[j0:j0 + _lib.SIM_MAX_SEGS]
            segs = (_lib.SimSeg * len(chunk))(*[_lib.SimSeg(t.data_ptr(), t.numel()) for t in chunk])
            _lib.check(_lib.lib().pk2_sim_gain_norm_seg(segs, len(chunk), _lib.ptr(peak), _lib.ptr(gain),
                                                        _lib.stream_ptr(mixed.device)))
        cfg['gain_norm_scale'] = gain                       # stays on the device (a CUDA float64 tensor)
    return mixed, pos_early, cfg


class MultiSourceSimulator:
    """Multiple speech source simulator, used to generate overlapping, multi-channel, noisy speech (reference
    simulation/simulation.py:237-296).  Channel-major device layout: sources and noises are 1-D CUDA float32 waveforms,
    their RIRs (C, k) tensors, `iso_noise_wav` a (C, m) tensor (generate_isotropic_noise); without RIRs the sources
    themselves are (C, n).  Returns (mixed_noisy (C, T), positioned_source_early_reverb | None, mask | None, sent_cfg);
    gen_mask=True forces the early reverberation and fills the third slot with the list of the sources' ideal binary masks,
    (N, F) CUDA float32 each (frame-major; MaskEstimator on channel 0, before the gain normalisation; `mask_seed` seeds the
    analyzer's dither, None draws one np.random.randint after every other draw).  The masks are computed by the
    `mask_estimator` given to the constructor, MaskEstimator(SpectrumAnalyzer(...)): the analysis (FFT size, window, dither)
    is the caller's choice, as the reference's config['analysis'] is; a simulator built without one keeps raising
    NotImplementedError for gen_mask=True;
    sent_cfg holds the draws (spr, start_sample_idx, dir_snr, dir_start, iso_snr, iso_start) and, as CUDA tensors, the
    mixer's `scale` and `gain_norm_scale`.  `snr_range` sets `global_snr` in the reference, which nothing reads: the
    directional SNR is uniform[0, 20] dB and the isotropic one uniform[10, 30] dB."""

    def __init__(self, array_geometry=None, use_rir=True, use_noise=True, snr_range=(0, 30), n_source_range=(2, 2),
                 spr_range=(-2.5, 2.5), mask_estimator=None):
        self.array_geometry, self.use_rir, self.use_noise = array_geometry, use_rir, use_noise
        self.snr_range, self.n_source_range = tuple(snr_range), tuple(n_source_range)
        self.mixer = Mixer(MixerConfig(spr_range))
        self.mask_estimator = mask_estimator   # what gen_mask=True computes the masks with

    def __call__(self, source_wavs, dir_noise_wavs=None, source_rirs=None, dir_noise_rirs=None, iso_noise_wav=None,
                 gen_mask=False, normalize_gain=True, get_early_reverb=False, rir_delays=None, fs=16000, mask_seed=None):
        if gen_mask:
            _require_mask_estimator(self.mask_estimator)
        mixed, early, cfg = _simulate(source_wavs, dir_noise_wavs, source_rirs, dir_noise_rirs, iso_noise_wav, normalize_gain,
                                      get_early_reverb or gen_mask, rir_delays, self.mixer, fs,
                                      mask_estimator=self.mask_estimator if gen_mask else None, mask_seed=mask_seed)
        return mixed, early, cfg.pop('mask', None), cfg


# ---------------------------------------------------------------------------------------------------------------------
# isotropic noise (reference simulation/_iso_noise_simulator.py)
# ---------------------------------------------------------------------------------------------------------------------
_hoth_freqs = [100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000]
_hoth_mag_db = [32.4, 30.9, 29.1, 27.6, 26, 24.4, 22.7, 21.1, 19.5, 17.8, 16.2, 14.6, 12.9, 11.3, 9.6, 7.8, 5.4, 2.6, -1.3, -6.6]
_hoth_index_1000_hz = 10
_hoth_index_4000_hz = 16
_speed_of_sound = 340       # m/s
ISO_NUM_POINTS = 512


@functools.lru_cache(maxsize=4)
def _sample_sphere(num_points):
    """(3, num_points) directions spiralling over the unit sphere (_iso_noise_simulator.py:28-50), host float64."""
    theta = np.zeros([num_points])
    phi = np.zeros([num_points])
    for k in range(0, num_points, 1):
        h = -1 + 2 * k / (num_points - 1)
        phi[k] = np.arccos(h)
        if k == 0 or k == num_points - 1:
            theta[k] = 0
        else:
            theta[k] = np.mod(theta[k - 1] + 3.6 / np.sqrt(num_points * (1 - h * h)), 2 * np.pi)
    return np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)])


@functools.lru_cache(maxsize=4)
def _sample_circle(num_points):
    """(3, num_points) directions on the unit circle of the horizontal plane (:82-94)."""
    phi = 2 * np.pi * np.arange(0, 1, 1 / num_points)
    return np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)])


def _not_a_knot_spline(x, y, xq):
    """The cubic spline through (x, y) with not-a-knot end conditions -- scipy's interp1d(kind='cubic') -- at xq, inside
    [x[0], x[-1]]."""
    n = x.shape[0]
    h = np.diff(x)
    A = np.zeros((n, n))
    r = np.zeros(n)
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
        r[i] = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
    A[0, 0], A[0, 1], A[0, 2] = h[1], -(h[0] + h[1]), h[0]                  # the third derivative is continuous at x[1]
    A[n - 1, n - 3], A[n - 1, n - 2], A[n - 1, n - 1] = h[n - 2], -(h[n - 3] + h[n - 2]), h[n - 3]     # ... and at x[n-2]
    M = np.linalg.solve(A, r)                                               # second derivatives at the knots
    i = np.clip(np.searchsorted(x, xq, side='right') - 1, 0, n - 2)
    t = xq - x[i]
    b = (y[i + 1] - y[i]) / h[i] - h[i] * (2 * M[i] + M[i + 1]) / 6
    return y[i] + t * (b + t * (M[i] / 2 + t * (M[i + 1] - M[i]) / (6 * h[i])))


def _get_hoth_mag(samp_rate, fft_size):
    """Magnitude of the Hoth noise spectrum (IEEE 269-2001) at the fft_size / 2 + 1 bins, 0 dB at 1 kHz, DC zeroed
    (:53-79).  Outside the table the reference's fill values: the first magnitude below; above, the last one at 16 kHz and
    the 5 kHz entry at 8 kHz."""
    if samp_rate not in (16000, 8000):
        raise ValueError('Can only generate Hoth noise for 16000 hz or 8000 hz sampling rates!')
    hoth_mag = np.asarray(_hoth_mag_db) - _hoth_mag_db[_hoth_index_1000_hz]
    hoth_mag = np.power(10, hoth_mag / 20)
    hoth_w = 2 * np.pi * np.asarray(_hoth_freqs) / samp_rate
    if samp_rate == 16000:
        x, y, fill = hoth_w, hoth_mag, (hoth_mag[0], hoth_mag[-1])
    else:
        x, y = hoth_w[0:_hoth_index_4000_hz + 1], hoth_mag[0:_hoth_index_4000_hz + 1]
        fill = (hoth_mag[0], hoth_mag[_hoth_index_4000_hz + 1])
    w = 2 * np.pi * np.arange(0, int(fft_size / 2) + 1, 1) / fft_size
    out = _not_a_knot_spline(x, y, np.clip(w, x[0], x[-1]))
    out[w < x[0]] = fill[0]
    out[w > x[-1]] = fill[1]
    out[0] = 0      # skip DC (0 Hz)
    return out


def _iso_setup(mic_xyz, N, samp_rate, type, spectrum):
    """Host float64 half: (fft_size, tau (C, P) in samples, g (F,) or None)."""
    mic_xyz = np.asarray(mic_xyz.detach().cpu().numpy() if isinstance(mic_xyz, torch.Tensor) else mic_xyz, dtype=np.float64)
    if mic_xyz.ndim != 2 or mic_xyz.shape[1] != 3 or mic_xyz.shape[0] < 1:
        raise ValueError("mic_xyz must be a (C, 3) matrix of microphone coordinates")
    if int(N) < 1 or int(N) > 2 ** 20:
        raise ValueError("N must be in [1, 2^20]")
    if samp_rate not in (16000, 8000):
        raise ValueError("samp_rate must be 16000 or 8000")
    fft_size = max(32, int(2 ** np.ceil(np.log2(int(N)))))       # (the transform starts at 2^5; the crop to N follows anyway)
    if type == 'sph':
        loc_xyz = _sample_sphere(ISO_NUM_POINTS)
    elif type == 'cyl':
        loc_xyz = _sample_circle(ISO_NUM_POINTS)
    else:
        raise ValueError("type must be 'sph' or 'cyl'")
    if spectrum == 'white':
        g = None
    elif spectrum == 'hoth':
        g = _get_hoth_mag(samp_rate, fft_size)
    else:
        raise ValueError("spectrum must be 'white' or 'hoth'")
    P_rel = mic_xyz - mic_xyz[0:1, :]
    tau = np.sum(P_rel[:, None, :] * loc_xyz.T[None, :, :], axis=2) * samp_rate / _speed_of_sound
    return fft_size, np.ascontiguousarray(tau), g


def iso_noise_spectra(mic_xyz, N, samp_rate, type='sph', spectrum='hoth', seed=None, draws=None, device=None):
    """The spectra X (C, fft_size / 2 + 1), a CUDA complex64 tensor, that generate_isotropic_noise transforms to the time
    domain: X[m, f] = (1 / sqrt(512)) sum_i g[f] Z_i[f] exp(-j tau[m, i] w_f) with the reference's bin scaling."""
    fft_size, tau, g = _iso_setup(mic_xyz, N, samp_rate, type, spectrum)
    _lib.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    C, P, F = tau.shape[0], tau.shape[1], fft_size // 2 + 1
    if draws is not None:
        draws = torch.as_tensor(draws)
        if tuple(draws.shape) != (P, F, 2) or draws.dtype != torch.float32:
            raise ValueError("draws must be a float32 array of shape (%d, %d, 2)" % (P, F))
        draws = _lib.h2d(draws.contiguous(), device)
        seed = 0
    elif seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    tau_d = _lib.h2d(tau.reshape(-1), device)
    g_d = _lib.h2d(np.ascontiguousarray(g), device) if g is not None else None
    X = torch.empty(C, F, 2, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pk2_iso_spectra(_lib.ptr(tau_d), _lib.ptr(g_d), _lib.ptr(draws), int(seed) & (2 ** 64 - 1), C, P, F,
                                              _lib.ptr(X), _lib.stream_ptr(device)))
    return torch.view_as_complex(X)


def iso_gauss(seed, points, bins, device=None):
    """The draws of the built-in generator: a CUDA float32 (points, bins, 2) tensor of standard normals, a pure function
    of (seed, point, bin) (tests and tools)."""
    _lib.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(int(points), int(bins), 2, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pk2_iso_gauss(int(seed) & (2 ** 64 - 1), int(points), int(bins), _lib.ptr(out),
                                            _lib.stream_ptr(device)))
    return out


def irfft_pow2(X):
    """numpy.fft.irfft along the last axis for a power-of-two length n = 2^5 .. 2^20: X is a CUDA complex64
    (rows, n / 2 + 1) tensor, the result a float32 (rows, n) tensor.  Hand-written transform (csrc/fft.hip)."""
    _lib.require_gpu()
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.complex64 and X.dim() == 2 and X.is_contiguous()):
        raise ValueError("irfft_pow2: expected a contiguous CUDA complex64 (rows, n / 2 + 1) tensor")
    rows, n = X.shape[0], 2 * (X.shape[1] - 1)
    out = torch.empty(rows, max(n, 1), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().pk2_irfft_pow2_f32(_lib.ptr(torch.view_as_real(X)), rows, n, _lib.ptr(out), _lib.stream_ptr(X.device)))
    return out


def generate_isotropic_noise(mic_xyz, N, samp_rate, type='sph', spectrum='hoth', seed=None, draws=None, device=None):
    """Isotropic noise for a microphone array (reference simulation/_iso_noise_simulator.py:97-160, after Habets & Gannot
    2007, with the Hoth spectral shaping), made on the device: a CUDA float32 (C, N) tensor, channel-major (the reference
    returns the same (C, N)).  mic_xyz: (C, 3) coordinates in metres; type 'sph' | 'cyl'; spectrum 'white' | 'hoth';
    samp_rate 16000 or 8000 (anything else is a ValueError, as is an unknown type or spectrum).

    The 2 x 512 x (fft_size / 2 + 1) normals come from a counter-based generator inside the kernel; `seed=None` draws one
    np.random.randint(0, 2**31 - 1) from numpy's global generator.  A seeded run is reproducible (bit for bit), but it is
    NOT the reference's noise for that numpy seed: the reference consumes 2 * 512 * F normals of the global stream.  For
    parity pass them as `draws`, a float32 (512, F, 2) array (real, imaginary)."""
    X = iso_noise_spectra(mic_xyz, N, samp_rate, type, spectrum, seed, draws, device)
    n = irfft_pow2(X)
    return n[:, :int(N)].contiguous() if n.shape[1] != int(N) else n


# ---------------------------------------------------------------------------------------------------------------------
# STFT, inverse STFT and ideal time-frequency masks (reference simulation/freq_analysis.py, simulation/mask.py)
# ---------------------------------------------------------------------------------------------------------------------
def _get_window(window, wlen):
    """The analysis window as host float64 (freq_analysis.py:9-38): a name, a callable or a vector."""
    if isinstance(window, str):
        if window == 'hamming':
            w = np.hamming(wlen)
        elif window == 'bartlett':
            w = np.bartlett(wlen)
        elif window in ('hann', 'hanning'):
            w = np.hanning(wlen)
        else:
            raise ValueError('cannot obtain window type {}'.format(window))
    elif callable(window):
        w = window(wlen)
    else:
        w = window.detach().cpu().numpy() if isinstance(window, torch.Tensor) else np.asarray(window)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.shape[0] != wlen:
        raise ValueError("the window has %d taps, frame_len is %d" % (w.shape[0], wlen))
    return w


def stft_num_frames(n, frame_len, frame_shift):
    """N = ceil((n + shift - len) / shift): the frames of the reference's _enframe(end='pad'), the signal zero-padded at
    its end.  A signal shorter than one frame is an error."""
    n, frame_len, frame_shift = int(n), int(frame_len), int(frame_shift)
    if frame_len < 1 or frame_shift < 1:
        raise ValueError("frame_len and frame_shift must be positive")
    if n < frame_len:
        raise ValueError("the signal (%d samples) is shorter than one frame (%d)" % (n, frame_len))
    return (n - frame_len + 2 * frame_shift - 1) // frame_shift


def _stft_rows(rows, fft_size, frame_len, frame_shift, window, seed=None, dither=None):
    """One launch (per 16 rows) for a list of 1-D CUDA float32 signals of one length -> float32 (R, N, F, 2), frame-major."""
    n, dev = rows[0].numel(), rows[0].device
    for x in rows:
        _check(x)
        if x.numel() != n or x.device != dev:
            raise ValueError("the signals of one STFT call differ in length or device")
    N = stft_num_frames(n, frame_len, frame_shift)
    R, F = len(rows), fft_size // 2 + 1
    if dither is not None:
        if not (isinstance(dither, torch.Tensor) and dither.is_cuda and dither.dtype == torch.float32 and dither.is_contiguous()
                and tuple(dither.shape) == (R, n)):
            raise ValueError("dither must be a contiguous CUDA float32 tensor of shape (%d, %d)" % (R, n))
    out = torch.empty(R, N, F, 2, dtype=torch.float32, device=dev)
    tab = (_lib.C.c_void_p * R)(*[x.data_ptr() for x in rows])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pk2_stft_f32(tab, R, n, int(fft_size), int(frame_len), int(frame_shift), _lib.ptr(window),
                                           _lib.ptr(dither), int(seed is not None), (int(seed) if seed is not None else 0) & (2 ** 64 - 1),
                                           _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


class SpectrumAnalyzer:
    """Short-time Fourier analysis and synthesis on the device (reference simulation/freq_analysis.py:231-266).  `config`
    overrides the attributes like the reference's; `dc_removal` is kept and unused, as there.  window: 'hamming',
    'hann' / 'hanning', 'bartlett', a callable or a vector (numpy float64 on the host, uploaded once per device).

    SPECTRA ARE FRAME-MAJOR: analyze returns (N, F) where the reference returns (F, N); `.transpose(-1, -2)` gives the
    reference's orientation.  N = ceil((n + frame_shift - frame_len) / frame_shift), the signal zero-padded at its end."""

    def __init__(self, config=None, fs=16000, fft_size=512, frame_len=400, frame_shift=160, window='hamming', do_dither=True,
                 dc_removal=False):
        self.fs, self.fft_size, self.frame_len, self.frame_shift = fs, fft_size, frame_len, frame_shift
        self.window, self.do_dither, self.dc_removal = window, do_dither, dc_removal
        if config is not None:
            for attr in config:
                setattr(self, attr, config[attr])
        self.n_bin = self.fft_size // 2 + 1
        self.frame_overlap = self.frame_len - self.frame_shift
        self._win = {}

    def window_taps(self):
        """the window as host float64"""
        return _get_window(self.window, int(self.frame_len))

    def _window(self, device):
        key = (torch.device(device), int(self.frame_len))
        if key not in self._win:
            self._win[key] = _lib.h2d(self.window_taps().astype(np.float32), device)
        return self._win[key]

    def num_frames(self, n):
        return stft_num_frames(n, self.frame_len, self.frame_shift)

    def _dither_args(self, seed, dither):
        if dither is not None or not self.do_dither:
            return None, dither
        return (int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)), None

    def _analyze_rows(self, rows, seed=None, dither=None):
        seed, dither = self._dither_args(seed, dither)
        return _stft_rows(rows, self.fft_size, self.frame_len, self.frame_shift, self._window(rows[0].device), seed, dither)

    def analyze(self, signal, seed=None, dither=None):
        """signal: (n,) or (R, n) CUDA float32 -> complex64 (N, F) or (R, N, F).

        With do_dither the reference adds np.random.normal(0, 1e-5) to every sample.  Here the normals come from the
        counter-based generator inside the kernel (simulation.iso_gauss(seed, R, ceil(n / 2)).view(R, -1)[:, :n] is the
        draw array, added as x + 1e-5 * z); `seed=None` draws one np.random.randint(0, 2**31 - 1) per call.  A seeded run is
        reproducible (bit for bit), but it is NOT the reference's dither for that numpy seed: the reference consumes n
        normals of the global stream.  For parity pass them as `dither`, a CUDA float32 tensor of the signal's shape
        that is added as it stands (and replaces the generator whatever do_dither is)."""
        _lib.require_gpu()
        one_d = signal.dim() == 1
        sig = _check_mc(signal.view(1, -1) if one_d else signal, "signal")
        if dither is not None:
            dither = dither.view(1, -1) if dither.dim() == 1 else dither
        spec = torch.view_as_complex(self._analyze_rows(list(sig.unbind(0)), seed, dither))
        return spec[0] if one_d else spec

    def log_spec(self, signal, seed=None, dither=None):
        return torch.log(torch.abs(self.analyze(signal, seed, dither)))

    def synthesize(self, stft_matrix):
        """The reference's istft(center=False): complex64 (N, F) or (R, N, F) -> float32 (fft_size + frame_shift (N - 1),)
        or (R, ...): overlap-add of the frames' inverse transforms divided by the summed analysis window where that sum
        exceeds 1e-10 (no synthesis window)."""
        _lib.require_gpu()
        X = stft_matrix
        if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.complex64 and X.dim() in (2, 3)):
            raise ValueError("synthesize: expected a CUDA complex64 (N, F) or (R, N, F) tensor")
        one_d = X.dim() == 2
        X = (X.unsqueeze(0) if one_d else X).contiguous()
        R, N, F = X.shape
        if F != self.fft_size // 2 + 1:
            raise ValueError("synthesize: %d bins, fft_size / 2 + 1 = %d" % (F, self.fft_size // 2 + 1))
        work = torch.empty(R, N, self.fft_size, dtype=torch.float32, device=X.device)
        out = torch.empty(R, self.fft_size + self.frame_shift * (N - 1), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            _lib.check(_lib.lib().pk2_istft_f32(_lib.ptr(torch.view_as_real(X)), R, N, int(self.fft_size), int(self.frame_len),
                                                int(self.frame_shift), _lib.ptr(self._window(X.device)), _lib.ptr(work),
                                                _lib.ptr(out), _lib.stream_ptr(X.device)))
        return out[0] if one_d else out


def mask_count_threshold(power, energy_threshold=0.997):
    """The cutoff of the 'count' clean mask (reference simulation/mask.py:75-79) for a CUDA float32 array of non-negative
    powers, (m,) or (S, m): with the values sorted ascending and summed cumulatively (float64), v* = the last value whose
    inclusive sum is < (1 - energy_threshold) * total; the clean mask is power > v*.  Returns a CUDA float32 (3,) or
    (S, 3) tensor (v, strict, v*): keep power > v when strict is 1, power >= v when it is 0 (v* is then the largest value
    below v).  Where the reference raises IndexError (no value satisfies the inequality) the result is (min, 0, 0):
    everything is kept."""
    _lib.require_gpu()
    one_d = power.dim() == 1
    p = _check_mc(power.view(1, -1) if one_d else power, "power")
    S, m = p.shape
    L = _lib.lib()
    nbytes = L.pk2_mask_count_workspace_bytes(S)
    work = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(S, 3, dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(L.pk2_mask_count_threshold(_lib.ptr(p), S, m, float(energy_threshold), _lib.ptr(work), nbytes, _lib.ptr(out),
                                              _lib.stream_ptr(p.device)))
    return out[0] if one_d else out


class MaskEstimator:
    """Ideal time-frequency masks from parallel clean / distorted waveforms (reference simulation/mask.py): 1 where a bin
    is dominated by the clean signal.  Binary: 10 log10(P_c / max(P_n, eps)) > snr_threshold with P_c = |C|^2 and
    P_n = |D - C|^2; soft: min(1, P_c / |D|^2).  Times the clean mask ('count': the loudest bins that hold 99.7 % of the
    clean energy; 'floor' is unfinished in the reference -> NotImplementedError; anything else: all ones) and the
    per-frame `vad > 0.5` (the reference's smoothing of it cannot run and its result is never used).  Masks are
    FRAME-MAJOR (N, F) like the analyzer's spectra.  `last_threshold` keeps the 'count' cutoffs of the last call, a CUDA
    float32 (S, 3) tensor (v, strict, v*) (see mask_count_threshold)."""

    def __init__(self, analyzer, snr_threshold=0.5, clean_mask_type='count', clean_mask_energy_threshold=0.997):
        self._analyzer = analyzer
        self._snr_threshold = snr_threshold
        self._clean_mask_type = clean_mask_type
        self._clean_mask_energy_threshold = clean_mask_energy_threshold
        self.last_threshold = None

    def get_mask_from_parallel_data(self, clean, distorted, vad=None, use_soft_mask=False, seed=None, dither=None):
        """clean: (n,) CUDA float32, or a list / an (S, n) batch of them; distorted: (n,).  Returns float32 (N, F), or
        (S, N, F) for a list or a batch.  All S + 1 signals go through one STFT launch; with the analyzer's dither they
        are its rows 0 .. S (the clean ones first), so clean and distorted get different dither: `seed` / `dither` as in
        SpectrumAnalyzer.analyze, `dither` of shape (S + 1, n).  vad: (N,) per frame, CUDA or host."""
        if self._clean_mask_type == 'floor':
            raise NotImplementedError("clean_mask_type='floor' is not implemented (nor is it in the reference)")
        _lib.require_gpu()
        single = isinstance(clean, torch.Tensor) and clean.dim() == 1
        rows = [clean] if single else list(clean.unbind(0) if isinstance(clean, torch.Tensor) else clean)
        S = len(rows)
        if S < 1:
            raise ValueError("no clean signal")
        spec = self._analyzer._analyze_rows(rows + [distorted], seed, dither)           # (S + 1, N, F, 2)
        N, F, dev = spec.shape[1], spec.shape[2], spec.device
        L, stream = _lib.lib(), _lib.stream_ptr(dev)
        thr = None
        with torch.cuda.device(dev):
            if self._clean_mask_type == 'count':
                power = torch.empty(S, N * F, dtype=torch.float32, device=dev)
                _lib.check(L.pk2_mask_power(_lib.ptr(spec), S * N * F, _lib.ptr(power), stream))
                thr = mask_count_threshold(power, self._clean_mask_energy_threshold)
            self.last_threshold = thr
            if vad is not None:
                vad = torch.as_tensor(vad)
                vad = _lib.h2d(vad.to(torch.float32).reshape(-1), dev).contiguous()
                if vad.numel() != N:
                    raise ValueError("vad has %d entries for %d frames" % (vad.numel(), N))
            mask = torch.empty(S, N, F, dtype=torch.float32, device=dev)
            factor = float(np.float32(10.0 ** (float(self._snr_threshold) / 10.0)))
            _lib.check(L.pk2_mask_ibm(_lib.ptr(spec), _lib.ptr(spec[S]), S, N, F, factor, int(bool(use_soft_mask)), _lib.ptr(thr),
                                      _lib.ptr(vad), _lib.ptr(mask), stream))
        return mask[0] if single else mask
