"""What beamform.py, dereverb.py and cgmm.py share: the ctypes tables of a ragged launch and the argument checks."""
import ctypes as C
import math

import numpy as np
import torch


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _frames(frames):
    return (C.c_int32 * len(frames))(*frames)


def _as_list(x, who):
    """(list, was a list)"""
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError("%s: the list of utterances is empty" % who)
        return list(x), True
    return [x], False


def _int_arg(v, lo, hi, who, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
    return int(v)


def _diag_load_arg(diag_load, who):
    if isinstance(diag_load, bool) or not isinstance(diag_load, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(diag_load)) or float(diag_load) < 0:
        raise ValueError("%s: diag_load must be a finite number >= 0, got %r" % (who, diag_load))
    return float(diag_load)


def _check_specs(spec, who, max_channels):
    """A spectrum or a list of them -> (list, was a list, C, F, device): contiguous CUDA complex64 (C, N, F), common C and F"""
    specs, many = _as_list(spec, who)
    for i, s in enumerate(specs):
        if not (isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.complex64 and s.dim() == 3 and s.is_contiguous()
                and s.numel() > 0):
            raise ValueError("%s: utterance %d: expected a contiguous CUDA complex64 (C, N, F) spectrum" % (who, i))
        if s.shape[0] != specs[0].shape[0] or s.shape[2] != specs[0].shape[2] or s.device != specs[0].device:
            raise ValueError("%s: utterance %d is (C, F) = (%d, %d) on %s, the first one (%d, %d) on %s"
                             % (who, i, s.shape[0], s.shape[2], s.device, specs[0].shape[0], specs[0].shape[2], specs[0].device))
    if specs[0].shape[0] > max_channels:
        raise ValueError("%s: %d channels, at most %d" % (who, specs[0].shape[0], max_channels))
    return specs, many, specs[0].shape[0], specs[0].shape[2], specs[0].device


def analyze_channels(analyzer, wav, who, max_channels):
    """(C, n) CUDA float32 -> complex64 (C, N, F) with the analyzer's FFT size, frame and window, without dither"""
    from . import simulation
    wav = simulation._check_mc(wav, "%s: wav" % who)
    if wav.shape[0] > max_channels:
        raise ValueError("%s: wav has %d channels, at most %d" % (who, wav.shape[0], max_channels))
    return torch.view_as_complex(simulation._stft_rows(list(wav.unbind(0)), analyzer.fft_size, analyzer.frame_len,
                                                       analyzer.frame_shift, analyzer._window(wav.device)))
