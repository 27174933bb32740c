"""Restatement of the reference's multi-channel / multi-source simulation -- TEST INFRASTRUCTURE ONLY (tests/ and
tools/ import it; the product path never does).

Restates in numpy, float64 by default, what the reference's simulation package computes beyond one source and one
channel (simulation/_distorter.py `Distorter.apply_rir` with a (T, C) RIR and its early reverberation, `add_noise`
with both placements; simulation/_mixer.py `Mixer`; simulation/_iso_noise_simulator.py `generate_isotropic_noise`;
simulation/simulation.py `_Simulator.simulate` as its text means it), in the device's CHANNEL-MAJOR layout: signals
are (C, T), RIRs (C, k).  `dtype=np.float32` runs the same arithmetic in single precision (numpy 2 keeps float32 /
complex64 through np.fft): 4 x its error against the float64 result is the tolerance of the float32 device kernels.

PINNED: tests/golden/simulation_mc.npz holds outputs of the reference's own code (tools/gen_golden_simmc.py);
tests/test_simmc_host.py checks this file against them to 1e-12.  The golden file stores no inputs: they are made
here from seeds with numpy's frozen legacy generator (`inputs_*`), rounded to float32.
"""
import numpy as np

NUM_POINTS = 512
SPEED_OF_SOUND = 340
HOTH_FREQS = [100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000]
HOTH_MAG_DB = [32.4, 30.9, 29.1, 27.6, 26, 24.4, 22.7, 21.1, 19.5, 17.8, 16.2, 14.6, 12.9, 11.3, 9.6, 7.8, 5.4, 2.6, -1.3, -6.6]


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/golden/simulation_mc.npz and their inputs
# ---------------------------------------------------------------------------------------------------------------------
REVERB_CASES = {"rev_a": dict(seed=101, n=1500, k=1500, C=3, delay=7),      # k crosses the 1024-tap stage, cut = 647
                "rev_b": dict(seed=102, n=1100, k=257, C=3, delay=1)}       # k shorter than the early cut
MIXER_CASE = dict(seed=201, lengths=(4000, 2500, 4000), C=2, spr=(1.5, -2.0), draw_seed=31)
NOISE_CASES = {"rep_short": dict(seed=301, n=4000, m=1300, C=2, snr=7.5, draw_seed=41, scheme="repeat_noise"),
               "rep_long": dict(seed=302, n=3000, m=9000, C=2, snr=15.0, draw_seed=42, scheme="repeat_noise"),
               "rep_equal": dict(seed=303, n=2048, m=2048, C=2, snr=0.0, draw_seed=43, scheme="repeat_noise"),
               "smp_short": dict(seed=304, n=5000, m=1800, C=3, snr=7.5, draw_seed=11, scheme="sample_noise"),
               "smp_long": dict(seed=305, n=3000, m=9000, C=3, snr=15.0, draw_seed=12, scheme="sample_noise"),
               "smp_equal": dict(seed=306, n=2048, m=2048, C=3, snr=0.0, draw_seed=13, scheme="sample_noise")}
ISO_MICS = np.array([[0.0, 0.0, 0.0], [0.05, 0.01, 0.0], [-0.02, 0.04, 0.03]])     # not collinear, out of the horizontal plane
ISO_CASES = {"iso_sph_white": dict(N=3000, fs=16000, type="sph", spectrum="white", seed=51),
             "iso_cyl_hoth": dict(N=3000, fs=16000, type="cyl", spectrum="hoth", seed=52),
             "iso_sph_hoth": dict(N=2048, fs=16000, type="sph", spectrum="hoth", seed=53),
             "iso_cyl_white": dict(N=2048, fs=16000, type="cyl", spectrum="white", seed=54),
             "iso_hoth_8k": dict(N=2048, fs=8000, type="sph", spectrum="hoth", seed=55)}


def make_wav(rs, n, amp, C=None):
    """AR(1)-coloured noise scaled to a peak of `amp`, float32; (n,) or (C, n)."""
    x = rs.standard_normal((C or 1, n))
    y = np.zeros_like(x)
    for i in range(1, n):
        y[:, i] = x[:, i] + 0.9 * y[:, i - 1]
    y = (amp * y / np.abs(y).max()).astype(np.float32)
    return y if C else y[0]


def make_rir(rs, k, delay, C):
    """(C, k) float32: a unit direct path at `delay` (+ 2 samples per further channel) and a decaying tail.  The
    reference reads the delay from channel 0 only."""
    r = np.zeros((C, k))
    for c in range(C):
        d = min(delay + 2 * c, k - 2)
        tail = np.arange(k - d - 1)
        r[c, d] = 1.0
        r[c, d + 1:] = 0.4 * rs.standard_normal(k - d - 1) * np.exp(-tail / (k / 6.0))
    return r.astype(np.float32)


def inputs_reverb(name):
    c = REVERB_CASES[name]
    rs = np.random.RandomState(c["seed"])
    return make_wav(rs, c["n"], 0.3), make_rir(rs, c["k"], c["delay"], c["C"])


def inputs_mixer():
    c = MIXER_CASE
    rs = np.random.RandomState(c["seed"])
    sig = [make_wav(rs, n, 0.1 * (i + 2), c["C"]) for i, n in enumerate(c["lengths"])]
    sig2 = [make_wav(rs, n, 0.05 * (i + 2), c["C"]) for i, n in enumerate(c["lengths"])]
    return sig, sig2


def inputs_noise(name):
    c = NOISE_CASES[name]
    rs = np.random.RandomState(c["seed"])
    return make_wav(rs, c["n"], 0.4, c["C"]), make_wav(rs, c["m"], 0.1, c["C"])


def legacy_draws(seed, F, P=NUM_POINTS):
    """The reference's draws under np.random.seed(seed): normal(0, 1, F) twice per direction, real part first
    (_iso_noise_simulator.py:142), as a float64 (P, F, 2) array."""
    rs = np.random.RandomState(seed)
    out = np.empty((P, F, 2))
    for i in range(P):
        out[i, :, 0] = rs.normal(0, 1, F)
        out[i, :, 1] = rs.normal(0, 1, F)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Distorter
# ---------------------------------------------------------------------------------------------------------------------
def fftconvolve_rows(a, b):
    """_fftconvolve1d along the last axis: a (C, k), b (n,) -> (C, k + n - 1), through rfft of a fast length."""
    from scipy.fft import next_fast_len
    rlen = a.shape[-1] + b.shape[-1] - 1
    nfft = next_fast_len(int(rlen))
    return np.fft.irfft(np.fft.rfft(a, nfft, axis=-1) * np.fft.rfft(b, nfft), nfft, axis=-1)[..., :rlen]


def apply_rir(wav, rir, fs=16000, get_early_reverb=False, dtype=np.float64, delay=None):
    """Distorter.apply_rir(sync=True): every channel is cut at the delay of channel 0.  Returns (reverb, early | None)."""
    wav, rir = np.asarray(wav, dtype), np.asarray(rir, dtype)
    n, k = wav.shape[0], rir.shape[1]
    delay = int(np.argmax(rir[0])) if delay is None else int(delay)
    reverb = fftconvolve_rows(rir, wav)[:, delay - 1:delay + n - 1]
    early = None
    if get_early_reverb:
        cut = int(np.minimum(k, 0.04 * fs + delay))
        early = fftconvolve_rows(rir[:, :cut], wav)[:, delay - 1:delay + n - 1]
    return reverb, early


def noise_scale(signal, noise, snr):
    return np.sqrt(np.mean(signal ** 2) / np.mean(noise ** 2) * 10 ** ((-snr) / 10))


def place_noise(noise, n, start, scheme):
    """The placed noise (C, n) for a drawn start."""
    m = noise.shape[1]
    if scheme == "repeat_noise":
        if m < n:
            noise = np.tile(noise, (1, int(np.ceil(n / m))))
        return noise[:, start:start + n]
    if m <= n:
        out = np.zeros((noise.shape[0], n), noise.dtype)
        out[:, start:start + m] = noise
        return out
    return noise[:, start:start + n]


def draw_noise_start(n, m, scheme):
    """The reference's draw from numpy's global generator (none where it makes none)."""
    if scheme == "repeat_noise":
        n_sample = int(np.ceil(n / m)) * m if m < n else m
        return 0 if n_sample == n else int(np.random.randint(0, high=n_sample - n, size=1)[0])
    n_extra = abs(n - m)
    return int(np.random.randint(0, high=n_extra, size=1)[0]) if n_extra > 0 else 0


def add_noise(signal, noise, snr, start, scheme, dtype=np.float64):
    signal, noise = np.asarray(signal, dtype), np.asarray(noise, dtype)
    return signal + place_noise(noise * dtype(noise_scale(signal, noise, snr)), signal.shape[1], start, scheme)


# ---------------------------------------------------------------------------------------------------------------------
# Mixer
# ---------------------------------------------------------------------------------------------------------------------
def mix(signals, spr, starts, signal2=None, dtype=np.float64):
    """Mixer.mix_signals for drawn starts: (mixed (C, T), scale (n,), positioned_source2 | None)."""
    signals = [np.asarray(x, dtype) for x in signals]
    T, C = max(x.shape[1] for x in signals), signals[0].shape[0]
    spr = np.insert(np.asarray(spr, np.float64), 0, 0)
    p_ref = np.mean(signals[0] ** 2)
    scale = np.array([np.sqrt(p_ref / np.mean(x ** 2) * 10 ** (spr[i] / 10)) for i, x in enumerate(signals)])
    mixed = np.zeros((C, T), dtype)
    pos2 = [] if signal2 is not None else None
    for i, x in enumerate(signals):
        mixed[:, starts[i]:starts[i] + x.shape[1]] += x * dtype(scale[i])
        if signal2 is not None:
            p = np.zeros((C, T), dtype)
            p[:, starts[i]:starts[i] + x.shape[1]] = np.asarray(signal2[i], dtype) * dtype(scale[i])
            pos2.append(p)
    return mixed, scale, pos2


def draw_mix_starts(lengths):
    T = max(lengths)
    return [int(np.random.randint(0, high=T - n, size=1)[0]) if n < T else 0 for n in lengths]


# ---------------------------------------------------------------------------------------------------------------------
# _Simulator.simulate as its text means it (the reference stops at an undefined name with several sources or an
# isotropic noise); draws from numpy's global generator in its textual order
# ---------------------------------------------------------------------------------------------------------------------
def simulate(source_wavs, dir_noise_wavs=(), source_rirs=None, dir_noise_rirs=(), iso_noise_wav=None, normalize_gain=True,
             get_early_reverb=False, spr_range=(-2.5, 2.5), fs=16000, dtype=np.float64):
    cfg = {}
    n_source = len(source_wavs)
    if source_rirs is not None:
        rv = [apply_rir(w, r, fs, get_early_reverb, dtype) for w, r in zip(source_wavs, source_rirs)]
        reverb, early = [a for a, _ in rv], [b for _, b in rv]
        noises = [apply_rir(w, r, fs, False, dtype)[0] for w, r in zip(dir_noise_wavs, dir_noise_rirs)]
    else:
        reverb = [np.asarray(w, dtype) for w in source_wavs]
        early = [x.copy() for x in reverb]
        noises = [np.asarray(w, dtype) for w in dir_noise_wavs]
    if n_source == 1:
        mixed, pos_early = reverb[0].copy(), early
    else:
        cfg["spr"] = np.random.uniform(low=float(spr_range[0]), high=float(spr_range[1]), size=n_source - 1)
        cfg["start_sample_idx"] = draw_mix_starts([x.shape[1] for x in reverb])
        mixed, cfg["scale"], pos_early = mix(reverb, cfg["spr"], cfg["start_sample_idx"], early if get_early_reverb else None, dtype)
    if noises:
        cfg["dir_snr"] = np.random.uniform(low=0.0, high=20.0, size=len(noises))
        cfg["dir_start"] = []
        for i, nz in enumerate(noises):
            cfg["dir_start"].append(draw_noise_start(mixed.shape[1], nz.shape[1], "sample_noise"))
            mixed = add_noise(mixed, nz, cfg["dir_snr"][i], cfg["dir_start"][i], "sample_noise", dtype)     # the aliasing
    if iso_noise_wav is not None:
        cfg["iso_snr"] = np.random.uniform(low=10.0, high=30.0, size=1)
        cfg["iso_start"] = draw_noise_start(mixed.shape[1], iso_noise_wav.shape[1], "repeat_noise")
        mixed = add_noise(mixed, iso_noise_wav, cfg["iso_snr"][0], cfg["iso_start"], "repeat_noise", dtype)
    if not get_early_reverb:
        pos_early = None
    if normalize_gain:
        g = 0.5 / np.max(np.abs(mixed))
        mixed = mixed * g
        if pos_early is not None:
            pos_early = [x * g for x in pos_early]
        cfg["gain_norm_scale"] = float(g)
    return mixed, pos_early, cfg


# ---------------------------------------------------------------------------------------------------------------------
# isotropic noise
# ---------------------------------------------------------------------------------------------------------------------
def sample_sphere(num_points=NUM_POINTS):
    theta, phi = np.zeros([num_points]), np.zeros([num_points])
    for k in range(num_points):
        h = -1 + 2 * k / (num_points - 1)
        phi[k] = np.arccos(h)
        theta[k] = 0 if k == 0 or k == num_points - 1 else np.mod(theta[k - 1] + 3.6 / np.sqrt(num_points * (1 - h * h)), 2 * np.pi)
    loc = np.zeros([3, num_points])
    for k in range(num_points):
        loc[:, k] = [np.sin(phi[k]) * np.cos(theta[k]), np.sin(phi[k]) * np.sin(theta[k]), np.cos(phi[k])]
    return loc


def sample_circle(num_points=NUM_POINTS):
    phi = 2 * np.pi * np.arange(0, 1, 1 / num_points)
    loc = np.zeros([3, len(phi)])
    for k in range(num_points):
        loc[:, k] = [np.cos(phi[k]), np.sin(phi[k]), 0]
    return loc


def hoth_mag(samp_rate, fft_size):
    """_get_hoth_mag through scipy's interp1d, as the reference computes it."""
    import scipy.interpolate as interp
    mag = np.power(10, (np.asarray(HOTH_MAG_DB) - HOTH_MAG_DB[10]) / 20)
    hw = 2 * np.pi * np.asarray(HOTH_FREQS) / samp_rate
    if samp_rate == 16000:
        f = interp.interp1d(hw, mag, kind="cubic", bounds_error=False, fill_value=(mag[0], mag[-1]))
    else:
        f = interp.interp1d(hw[0:17], mag[0:17], kind="cubic", bounds_error=False, fill_value=(mag[0], mag[17]))
    out = f(2 * np.pi * np.arange(0, fft_size // 2 + 1, 1) / fft_size)
    out[0] = 0
    return out


def iso_tau(mic_xyz, samp_rate, type):
    """(C, P) delays in samples of every direction at every microphone against microphone 0"""
    loc = sample_sphere() if type == "sph" else sample_circle()
    P_rel = np.asarray(mic_xyz, np.float64) - np.asarray(mic_xyz, np.float64)[0]
    return np.array([[np.sum(P_rel[m] * loc[:, i]) * samp_rate / SPEED_OF_SOUND for i in range(loc.shape[1])]
                     for m in range(P_rel.shape[0])])


def iso_spectra(mic_xyz, N, samp_rate, type, spectrum, draws, dtype=np.float64):
    """X (C, F) before the inverse transform, from the draws (P, F, 2)."""
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    fft_size = max(32, int(2 ** np.ceil(np.log2(N))))
    half = fft_size // 2
    tau = iso_tau(mic_xyz, samp_rate, type)
    g = dtype(1) if spectrum == "white" else hoth_mag(samp_rate, fft_size).astype(dtype)
    w = (2 * np.pi * np.arange(0, half + 1, 1) / fft_size).astype(dtype)
    X = np.zeros([tau.shape[0], half + 1], dtype=cdtype)
    for i in range(tau.shape[1]):
        x_this = (g * (draws[i, :, 0].astype(dtype) + 1j * draws[i, :, 1].astype(dtype))).astype(cdtype)
        X[0] += x_this
        for m in range(1, tau.shape[0]):
            X[m] += x_this * np.exp(-1j * dtype(tau[m, i]) * w).astype(cdtype)
    X = X / dtype(np.sqrt(tau.shape[1]))
    X[:, 0] = dtype(np.sqrt(fft_size)) * np.real(X[:, 0])
    X[:, half] = dtype(np.sqrt(fft_size)) * np.real(X[:, half])
    X[:, 1:half] = dtype(np.sqrt(half)) * X[:, 1:half]
    return X


def iso_noise(mic_xyz, N, samp_rate, type, spectrum, draws, dtype=np.float64):
    X = iso_spectra(mic_xyz, N, samp_rate, type, spectrum, draws, dtype)
    return np.fft.irfft(X, 2 * (X.shape[1] - 1), axis=1)[:, :N]


def iso_coherence(tau, w):
    """The quadrature (1 / P) sum_i cos(tau_i w) of the field's spatial coherence between two microphones."""
    return np.cos(np.outer(w, tau)).mean(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the counter-based generator of the device (csrc/iso_noise.hip: iso_gauss)
# ---------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def gauss_host(seed, points, bins, dtype=np.float64, counters=None):
    """(points, bins, 2) standard normals, the pure function of (seed, point, bin) of the kernel: splitmix64 finaliser of
    seed * 0xD1342543DE82EF95 + point * bins + bin, u = (k + 0.5) 2^-24 from its bits 63..40 and 39..16, Box-Muller.
    `counters`: only these flat indices (any shape) instead of all."""
    with np.errstate(over="ignore"):
        ctr = np.arange(points * bins, dtype=np.uint64) if counters is None else np.asarray(counters, np.uint64)
        z = _mix64(np.uint64(seed) * np.uint64(0xD1342543DE82EF95) + ctr)
    k1 = (z >> np.uint64(40)).astype(np.int64)
    k2 = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)
    if dtype == np.float64:
        lg = np.log((k1 + 0.5) * 2.0 ** -24)
        ang = 2 * np.pi * (k2 + 0.5) * 2.0 ** -24
    else:           # the kernel's float32 steps: the upper half of u1 through log1p of an exact argument
        f = np.float32
        lo = np.log((k1.astype(f) + f(0.5)) * f(2.0 ** -24))
        hi = np.log1p(-((2 ** 24 - 1 - k1).astype(f) + f(0.5)) * f(2.0 ** -24))
        lg = np.where(k1 < 2 ** 23, lo, hi).astype(f)
        ang = (f(np.pi) * ((k2.astype(f) + f(0.5)) * f(2.0 ** -23))).astype(f)
    r = np.sqrt(dtype(-2) * lg)
    out = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1).astype(dtype)
    return out.reshape(points, bins, 2) if counters is None else out
