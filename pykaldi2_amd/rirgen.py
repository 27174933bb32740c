"""Room impulse responses by the image method, generated on the device (reference simulation/_rirgen.py
`xp_rirgen`, method 1, which the reference wrote for cupy arrays), and the room / array / source draws that the
reference's simulation config provides for RIRs made on the fly (simulation/config.py `reverb.use_corpus`,
simulation/_geometry.py RoomConfig / ArrayPositionConfig / SoundSourceConfig, simulation/_sampling.py).

The host checks the arguments exactly as the reference does and forms one descriptor per item; the kernels
(csrc/rirgen.hip) make the candidate images, their windowed-sinc taps, the high-pass and each row's argmax.  Output
rows are CUDA float32, bit-reproducible from run to run (the taps are summed in 64-bit fixed point), and equal to the
reference's float32 result within the reference's own numpy-vs-cupy tolerance (atol = rtol = 1e-5).
"""
import math

import numpy as np
import torch

from . import _lib

_F64, _I64 = 16, 12          # PK2_RIR_F64 / PK2_RIR_I64 (include/pk2hip.h)
_PARTS_POINTS = 4096         # lattice points per workgroup of the tap kernel (a row's lattice is split into parts)


def t60_to_alpha(room, t60):
    """Sabine absorption coefficient of the walls for a reverberation time (reference _rirgen.py:4-9, c = 343)."""
    room = np.asarray(room, dtype=np.float64).reshape(-1)
    V = np.prod(room)
    c = 343
    S = 2 * (room[0] * room[2] + room[1] * room[2] + room[0] * room[1])
    return 24 * V * np.log(10) / (c * S * t60)


def min_t60_of_room(room):
    """1.1 x the T60 of fully absorbing walls (reference _rirgen.py:11-16, c = 343)."""
    room = np.asarray(room, dtype=np.float64).reshape(-1)
    V = np.prod(room)
    c = 343
    S = 2 * (room[0] * room[2] + room[1] * room[2] + room[0] * room[1])
    min_t60 = 24 * V * np.log(10) / (c * S)
    return min_t60 * 1.1


def _host(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def prepare(room, source_loc, mic_loc, c=340, fs=16000, t60=0.5, beta=None, nsamples=None, htw=None, hpfilt=True,
            habets_compat=False, method=1):
    """Host half of xp_rirgen: the reference's checks and exceptions, in its order, and the item's descriptor.
    No GPU is touched."""
    if method == 2:
        raise NotImplementedError("xp_rirgen method 2 (frequency-domain sum) is not implemented: the reference calls it "
                                  "untested and too slow; use method 1")
    if method != 1:
        raise ValueError("method must be 1")
    room = _host(room).reshape(3, 1)
    source_loc = _host(source_loc).reshape(3, -1)
    mic_loc = _host(mic_loc).reshape(3, -1)
    if beta is None and t60 is None:
        raise ValueError('Either t60 or beta array must be provided')
    elif beta is None:
        V = np.prod(room)
        S = 2 * (room[0] * room[2] + room[1] * room[2] + room[0] * room[1])
        alpha = 24 * V * np.log(10) / (c * S * t60)
        if alpha < 1:
            beta = np.ones(6, ) * np.sqrt(1 - alpha)
        else:
            raise ValueError('t60 value {} too small for the room'.format(t60))
    else:
        beta = _host(beta).reshape(-1)
        if np.max(beta) >= 1.0 or np.min(beta) <= 0.0:
            raise ValueError('beta array values should be in the interval (0,1).')
        if t60 is not None:
            print('Overwriting provided t60 value using provided beta array')
        alpha = 1 - beta ** 2
        V = np.prod(room)
        Se = 2 * (room[1] * room[2] * (alpha[0] + alpha[1]) + room[0] * room[2] * (alpha[2] + alpha[3]) +
                  room[0] * room[1] * (alpha[4] + alpha[5]))
        t60 = 24 * np.log(10.0) * V / (c * Se)
    if htw is None:
        htw = np.minimum(32, int(np.min(room) / 10 / c * fs))
    if habets_compat:
        htw = 64
    htw = int(htw)
    if not (np.all(room.T - mic_loc.T > 0) and np.all(room.T - source_loc.T > 0) and np.all(mic_loc.T > 0)
            and np.all(source_loc.T > 0)):
        raise ValueError('Room dimensions and source and mic locations are not compatible.')
    cTs = c / fs
    room_s, mic_s, src_s = room / cTs, mic_loc / cTs, source_loc / cTs
    if nsamples is None:
        nsamples = int(fs * np.asarray(t60).reshape(-1)[0])
    nsamples = int(nsamples)
    if nsamples < 1 or htw < 0:
        raise ValueError("nsamples must be positive and htw non-negative")
    c0 = 0.5 / c * fs                         # rough gain denominator offset; the rough gain at the origin is 1 / c0
    f = np.zeros(_F64)
    f[0:3] = room_s[:, 0]
    f[3:9] = beta
    f[9], f[10], f[11] = c0, (1.0 / c0) / 1.0e4, cTs
    if habets_compat:
        W = 2 * np.pi * 100 / fs
        R1 = np.exp(-W)
        B1 = 2 * R1 * np.cos(W)
        B2 = -R1 * R1
        A1 = -(1 + R1)
        f[12:16] = (A1, R1, -B1, -B2)          # b = [1, A1, R1], a = [1, -B1, -B2]
    half = []
    for q in range(3):
        nrefl = int(nsamples / room_s[q, 0])   # the reference's lattice bound
        half.append(min(nrefl, int(nsamples / (2 * room_s[q, 0])) + 1))     # beyond it the rough delay is >= nsamples
    return dict(f64=f, nsrc=source_loc.shape[1], nmic=mic_loc.shape[1], nsamples=nsamples, htw=htw,
                mode=2 if habets_compat else (1 if hpfilt else 0), pos=np.concatenate([src_s.T.reshape(-1), mic_s.T.reshape(-1)]),
                half=half)


class RirBatch:
    """The result of rirgen_batch: `rirs[i]` (nsrc, nmic, nsamples) and `delays[i]` (nsrc, nmic, int32, argmax of each
    row) are views of the flat device buffers `out` and `delay`."""

    def __init__(self, out, delay, rirs, delays):
        self.out, self.delay, self.rirs, self.delays = out, delay, rirs, delays


def rirgen_batch(items, c=340, fs=16000, device=None):
    """Many RIR items in one call.  `items`: dicts of xp_rirgen's per-item arguments (room, source_loc, mic_loc and
    optionally t60, beta, nsamples, htw, hpfilt, habets_compat, method); `c` and `fs` are shared.  Every item is
    checked on the host before the library is touched.  Makes no host synchronisation."""
    preps = [prepare(c=c, fs=fs, **it) for it in items]
    assert preps, "empty batch"
    _lib.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    seg = int(_lib.lib().pk2_rirgen_segment_samples())
    f64 = np.stack([p["f64"] for p in preps])
    i64 = np.zeros((len(preps), _I64), dtype=np.int64)
    pos, wg, row_item = [], [], []
    pos_off = out_off = row0 = 0
    for i, p in enumerate(preps):
        ns, rows = p["nsamples"], p["nsrc"] * p["nmic"]
        i64[i, :11] = (p["nsrc"], p["nmic"], ns, p["htw"], p["mode"], pos_off, out_off, row0) + tuple(p["half"])
        pos.append(p["pos"])
        npts = (2 * p["half"][0] + 1) * (2 * p["half"][1] + 1) * (2 * p["half"][2] + 1)
        parts = max(1, min(256, -(-npts // _PARTS_POINTS)))
        for r in range(rows):
            row_item.append((i, r))
            for s0 in range(0, ns, seg):
                wg.extend((i, r, part, parts, s0) for part in range(parts))
        pos_off += p["pos"].shape[0]
        out_off += rows * ns
        row0 += rows
    total, nrows = out_off, row0
    f64_d = _lib.h2d(np.ascontiguousarray(f64.reshape(-1)), device)
    i64_d = _lib.h2d(np.ascontiguousarray(i64.reshape(-1)), device)
    pos_d = _lib.h2d(np.concatenate(pos).astype(np.float64), device)
    wg_d = _lib.h2d(np.asarray(wg, dtype=np.int32).reshape(-1), device)
    ri_d = _lib.h2d(np.asarray(row_item, dtype=np.int32).reshape(-1), device)
    acc = torch.empty(total, dtype=torch.int64, device=device)
    out = torch.empty(total, dtype=torch.float32, device=device)
    delay = torch.empty(nrows, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pk2_rirgen(_lib.ptr(f64_d), _lib.ptr(i64_d), _lib.ptr(pos_d), _lib.ptr(wg_d), len(wg),
                                         _lib.ptr(ri_d), nrows, total, _lib.ptr(acc), _lib.ptr(out), _lib.ptr(delay),
                                         _lib.stream_ptr(device)))
    rirs, delays = [], []
    for i, p in enumerate(preps):
        o, r0, rows = int(i64[i, 6]), int(i64[i, 7]), p["nsrc"] * p["nmic"]
        rirs.append(out[o:o + rows * p["nsamples"]].view(p["nsrc"], p["nmic"], p["nsamples"]))
        delays.append(delay[r0:r0 + rows].view(p["nsrc"], p["nmic"]))
    return RirBatch(out, delay, rirs, delays)


def xp_rirgen(room, source_loc, mic_loc, c=340, fs=16000, t60=0.5, beta=None, nsamples=None, htw=None, hpfilt=True,
              habets_compat=False, method=1):
    """Room impulse responses of each source-microphone pair (reference _rirgen.py:18-182, same arguments and
    defaults): room (3, 1) metres, source_loc (3, nsrc), mic_loc (3, nmic), host arrays.  Returns a CUDA float32 tensor
    (nsrc, nmic, nsamples).  beta, when given, overrides t60; habets_compat sets htw = 64 and applies Habets' IIR
    high-pass instead of the 3-tap FIR (which the reference only allows with numpy)."""
    return rirgen_batch([dict(room=room, source_loc=source_loc, mic_loc=mic_loc, t60=t60, beta=beta, nsamples=nsamples,
                              htw=htw, hpfilt=hpfilt, habets_compat=habets_compat, method=method)], c=c, fs=fs).rirs[0]


# ---------------------------------------------------------------------------------------------------------------------
# draws of a room, an array position and source positions (reference simulation/_sampling.py with the default
# RoomConfig / ArrayPositionConfig / SoundSourceConfig of simulation/_geometry.py), numpy's global generator
# ---------------------------------------------------------------------------------------------------------------------
def _uniform(low, high):
    return np.random.uniform(low=float(low), high=float(high), size=1)[0]


def sample_room():
    """sample_room(RoomConfig().config): length, width ~ U[2.5, 20] m, height ~ U[2.5, 5] m."""
    room = np.zeros((3,))
    room[0] = _uniform(2.5, 20)
    room[1] = _uniform(2.5, 20)
    room[2] = _uniform(2.5, 5)
    return room


def sample_array_center(room):
    """sample_array_position(ArrayPositionConfig(zeros)) (use_gaussian False): ratios U[0.2, 0.8], U[0.2, 0.8],
    U[0.4, 0.6] of the room's length, width, height.  Returns (3, 1)."""
    ctr = np.zeros((3,))
    ctr[0] = _uniform(0.2, 0.8)
    ctr[1] = _uniform(0.2, 0.8)
    ctr[2] = _uniform(0.4, 0.6)
    return ctr.reshape(3, 1) * room.reshape(3, 1)


def sample_array(room, mic_positions):
    """sample_array_position(ArrayPositionConfig(mic_positions)) of the reference (simulation/_sampling.py:206-237,
    use_gaussian False): the array centre as sample_array_center draws it, and the microphones at centre + mic_positions
    (3, C) (the offsets of the array geometry from its centre).  Returns (array_ctr (3, 1), mic_position (3, C))."""
    mic_positions = np.asarray(mic_positions, dtype=np.float64)
    if mic_positions.ndim != 2 or mic_positions.shape[0] != 3:
        raise ValueError("mic_positions must be a (3, C) matrix")
    ctr = sample_array_center(np.asarray(room, dtype=np.float64))
    return ctr, ctr + mic_positions


def sample_sources(n_spk, room, array_center):
    """sample_source_position_by_random_coordinate(SoundSourceConfig().config, n_spk, room, array_center): x, y at least
    0.5 m from the walls, height ~ U[1, 2] m, at least 0.3 m from the array centre in the horizontal plane and 0.5 m from
    the sources placed before; at most 1000 trials per source.  Returns (3, n_spk)."""
    array_center = np.asarray(array_center, dtype=np.float64).reshape(-1)
    source_position = np.zeros((3, n_spk))
    for i in range(n_spk):
        cnt = 0
        while 1:
            cnt += 1
            x = _uniform(0.5, room[0] - 0.5)
            y = _uniform(0.5, room[1] - 0.5)
            z = _uniform(1, 2)
            curr_pos = np.asarray([x, y, z])
            if np.linalg.norm(curr_pos[:2] - array_center[:2]) >= 0.3:
                if i == 0 or (np.linalg.norm(curr_pos[:2, np.newaxis] - source_position[:2, :i], axis=0) >= 0.5).all():
                    source_position[:, i] = curr_pos[:]
                    break
            if cnt > 1000:
                raise Exception("Maximum number (1000) of trial finished but still not able to find acceptable position "
                                "for speaker position. ")
    return source_position


def sample_online_room(t60_range=(0.1, 0.5), n_src=2, mic_positions=None):
    """One room for an on-the-fly RIR, drawn in this order: the room; the T60 ~ U[t60_range], raised to
    min_t60_of_room(room) when below it (the reference would raise 't60 value too small' there instead); one mic at the
    array centre; `n_src` sources (speech first, then the directional noise).  Returns (room (3,), t60, mic (3, 1),
    sources (3, n_src)).  With `mic_positions` (3, C), the offsets of an array from its centre, the microphones are
    sample_array's (3, C) instead; the draws are the same."""
    room = sample_room()
    lo, hi = float(t60_range[0]), float(t60_range[1])
    t60 = float(np.random.uniform(low=lo, high=hi, size=1)[0])
    t60 = max(t60, float(min_t60_of_room(room)))
    if mic_positions is None:
        ctr = mic = sample_array_center(room)
    else:
        ctr, mic = sample_array(room, mic_positions)
    src = sample_sources(n_src, room, ctr[:, 0])
    return room, t60, mic, src
