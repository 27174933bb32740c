"""Restatement of the reference's STFT, inverse STFT and ideal-mask estimator -- TEST INFRASTRUCTURE ONLY (tests/ and
tools/ import it; the product path never does).

Restates in numpy, float64 by default, simulation/freq_analysis.py (`stft` / `istft` with center=False, `_enframe` with
end='pad') and simulation/mask.py (`MaskEstimator.get_mask_from_parallel_data`), in the device's FRAME-MAJOR layout:
spectra and masks are (N, F) where the reference's `analyze` returns (F, N).  `dtype=np.float32` runs the same arithmetic
in single precision (numpy 2 keeps float32 / complex64 through np.fft): 4 x its error against the float64 result is the
tolerance of the float32 device kernels.  `descent_threshold` is a numpy model of the device's radix descent for the
'count' clean mask's cutoff.

PINNED: tests/golden/simulation_mask.npz holds outputs of the reference's own code (tools/gen_golden_mask.py);
tests/test_mask_host.py checks this file against them.  The golden file stores no inputs: they are made here from seeds
with numpy's frozen legacy generator, rounded to float32.
"""
import numpy as np

# (seed, n, snr_db): the clean mask keeps 12-14 % of the bins, so both comparisons of the mask are exercised
MASK_CASES = {"m1": (1, 6000, 5), "m2": (2, 6000, 0), "m4": (4, 3055, 5), "m6": (6, 6000, 30), "m7": (7, 6000, -10)}
DITHER_SEED = 77            # np.random.seed before the reference's analyze calls (clean first, then distorted)
DEFAULT = dict(fft_size=512, frame_len=400, frame_shift=160, window="hamming")
# the configurations of the STFT / inverse STFT tests beyond the default one: name -> (config, n, seed)
STFT_CASES = {"hann64": (dict(fft_size=64, frame_len=64, frame_shift=16, window="hann"), 1000, 11),
              "bartlett32": (dict(fft_size=32, frame_len=20, frame_shift=7, window="bartlett"), 333, 12),
              "hamming1024": (dict(fft_size=1024, frame_len=600, frame_shift=200, window="hamming"), 5000, 13),
              "hamming4096": (dict(fft_size=4096, frame_len=4096, frame_shift=1024, window="hamming"), 9000, 14)}


def inputs(seed, n, snr_db):
    """(clean, distorted) float32: twelve amplitude-modulated sinusoids plus a noise floor, and white noise at snr_db."""
    r = np.random.RandomState(seed)
    t = np.arange(n) / 16000
    env = 0.5 * (1 + np.sin(2 * np.pi * 3 * t + r.uniform(0, 6)))
    clean = sum(r.uniform(.02, .1) * np.sin(2 * np.pi * f * t + r.uniform(0, 6)) for f in r.uniform(100, 7000, 12)) * env \
        + 1e-3 * r.standard_normal(n)
    noise = r.standard_normal(n)
    noise *= np.sqrt(np.mean(clean ** 2) / np.mean(noise ** 2) * 10 ** (-snr_db / 10))
    return clean.astype(np.float32), (clean + noise).astype(np.float32)


def get_window(window, wlen):
    if isinstance(window, str):
        return {"hamming": np.hamming, "bartlett": np.bartlett, "hann": np.hanning, "hanning": np.hanning}[window](wlen)
    return np.asarray(window(wlen) if callable(window) else window, dtype=np.float64)


def num_frames(n, frame_len, frame_shift):
    """_enframe(end='pad'): the signal is zero-padded at its end to a whole number of frames"""
    if n < frame_len:
        raise ValueError("the signal is shorter than one frame")
    return -(-(n + frame_shift - frame_len) // frame_shift)


def stft(y, fft_size=512, frame_len=400, frame_shift=160, window="hamming", dither=None, dtype=np.float64):
    """(N, F) complex: frame = (y + dither) * window, zero-extended to fft_size, bins 0 .. fft_size / 2."""
    y = np.asarray(y, dtype=dtype)
    if dither is not None:
        y = y + np.asarray(dither, dtype=dtype)
    N = num_frames(y.shape[0], frame_len, frame_shift)
    y = np.concatenate([y, np.zeros((N - 1) * frame_shift + frame_len - y.shape[0], dtype=dtype)])
    idx = np.arange(frame_len)[None, :] + frame_shift * np.arange(N)[:, None]
    frames = y[idx] * get_window(window, frame_len).astype(dtype)[None, :]
    return np.fft.fft(frames, n=fft_size, axis=1)[:, :fft_size // 2 + 1]


def istft(X, frame_len=400, frame_shift=160, window="hamming", small_float=1e-10, dtype=np.float64, **_):
    """(fft_size + shift (N - 1),): overlap-add of the frames' inverse transforms, divided by the summed analysis window
    (its frame_len taps only) where that sum exceeds small_float.  No synthesis window."""
    X = np.asarray(X)
    N, fft_size = X.shape[0], 2 * (X.shape[1] - 1)
    w = get_window(window, frame_len).astype(dtype)
    full = np.concatenate((X, X.conj()[:, -2:0:-1]), axis=1)
    frames = np.fft.ifft(full).real.astype(dtype)
    y = np.zeros(fft_size + frame_shift * (N - 1), dtype=dtype)
    ws = np.zeros_like(y)
    for f in range(N):
        y[f * frame_shift:f * frame_shift + fft_size] += frames[f]
        ws[f * frame_shift:f * frame_shift + frame_len] += w
    ok = ws > small_float
    y[ok] /= ws[ok]
    return y, ws


def count_threshold(power, energy_threshold=0.997):
    """mask.py:75-79: (v*, ok); ok False where the reference raises IndexError (no value satisfies the inequality)"""
    srt = np.sort(np.asarray(power).reshape(-1))
    cs = np.cumsum(srt)
    idx = np.where(cs < (1.0 - energy_threshold) * cs[-1])[0]
    return (srt[idx[-1]], True) if idx.size else (srt[0], False)


def count_mask(power, energy_threshold=0.997):
    v, ok = count_threshold(power, energy_threshold)
    return power > v if ok else np.ones(power.shape, bool)


def mask(clean, distorted, cfg=DEFAULT, dither=None, vad=None, use_soft_mask=False, snr_threshold=0.5, energy_threshold=0.997,
         dtype=np.float64):
    """get_mask_from_parallel_data, frame-major.  dither: None or (2, n) (clean, distorted).  Returns a dict: mask (N, F)
    float, snr_db, power_clean, v (the clean mask's cutoff)."""
    d = (None, None) if dither is None else dither
    C = stft(clean, dither=d[0], dtype=dtype, **cfg)
    D = stft(distorted, dither=d[1], dtype=dtype, **cfg)
    pc = np.abs(C) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        if use_soft_mask:
            snr = None
            m_snr = np.minimum(1, pc / np.abs(D) ** 2)
        else:
            snr = 10 * np.log10(pc / np.maximum(np.abs(D - C) ** 2, np.finfo(np.float32).eps))
            m_snr = snr > snr_threshold
    v, ok = count_threshold(pc, energy_threshold)
    m_clean = pc > v if ok else np.ones(pc.shape, bool)
    out = m_snr * m_clean
    vad_clean = np.ones((pc.shape[0], 1)) if vad is None else (np.asarray(vad).reshape(-1, 1) > 0.5)
    return dict(mask=out.astype(np.float32) * vad_clean.astype(np.float32), snr_db=snr, power_clean=pc, v=v, clean=m_clean)


def descent_threshold(power, energy_threshold=0.997):
    """numpy model of the device's radix descent (csrc/mask.hip) over float32 powers: (v, strict) -- keep power > v when
    strict, power >= v otherwise.  Four levels of 8 bits over the bit pattern; per level the buckets' float64 sums are
    walked in ascending order to the first one at whose end the running sum is not below tau."""
    p = np.ascontiguousarray(power, dtype=np.float32).reshape(-1)
    u = p.view(np.uint32)
    prefix, run, tau = 0, 0.0, None
    for level in range(4):
        shift = 24 - 8 * level
        sel = np.ones(u.shape, bool) if level == 0 else (u >> np.uint32(shift + 8)) == prefix
        b = ((u[sel] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        cnt = np.bincount(b, minlength=256)
        sums = np.array([p[sel][b == k].astype(np.float64).sum() if cnt[k] else 0.0 for k in range(256)])
        if level == 0:
            total = 0.0
            for k in range(256):
                total += sums[k]
            tau = (1.0 - energy_threshold) * total
        pick, before = 0, run
        for k in range(256):
            if cnt[k] == 0:
                continue
            pick, before = k, run
            if not run + sums[k] < tau:
                break
            run += sums[k]
        run, prefix = before, (prefix << 8) | pick
    v = np.array([prefix], np.uint32).view(np.float32)[0]
    return v, bool(run + np.float64(v) < tau)


THRESHOLD_NAMES = ["one", "two", "two_degenerate", "equal1000", "exact_tau", "per_bucket", "random", "large"]


def threshold_arrays():
    """name -> float32 array; integer-valued (or one value per bucket), so that every float64 sum is exact.  The cases of the
    threshold tests (host model and device)."""
    rs = np.random.RandomState(5)
    # cumulative sum equal to tau exactly: tau = fl(1 - 0.997) * total is not an integer in general, so take the energy
    # threshold 0.75: (1 - 0.75) * 400 = 100 = 30 + 70 exactly; the inequality is strict, so 70 is not below the cutoff
    exact = np.array([30, 70, 100, 200], dtype=np.float32)
    return {
        "one": (np.array([5.0], np.float32), 0.997),
        "two": (np.array([1000.0, 1.0], np.float32), 0.997),
        "two_degenerate": (np.array([2.0, 3.0], np.float32), 0.997),
        "equal1000": (np.full(1000, 7.0, np.float32), 0.997),
        "exact_tau": (exact, 0.75),
        # 2^-140 (subnormal) and one power of two in every further first-level bucket (exponent fields 2k, 2k + 1) up to 2^100
        "per_bucket": (np.ldexp(1.0, np.concatenate([[-140], np.arange(-124, 101, 2)])).astype(np.float32), 0.997),
        "random": (rs.randint(0, 5000, size=257 * 36).astype(np.float32), 0.997),
        "large": (rs.randint(0, 2 ** 20, size=2 ** 20 + 3).astype(np.float32), 0.997),
    }


def decide(power, v, strict):
    return power > v if strict else power >= v
