"""Device time of the multi-channel simulation, written to profiles/simmc_time.txt:

  * generate_isotropic_noise for a 7-microphone circular array (radius 4.25 cm plus the centre), N = 160000 (10 s)
  * one full simulation: 2 sources, 7 channels, 2 directional noises, 8000-tap RIRs, isotropic noise, early reverberation

each the median of 10 runs between device events after 2 warm-up runs, and next to them the CPU time of the same
isotropic call in numpy: the restatement tests/simmc_ref.py (the reference's loop), or the reference's own function
with --ref DIR (a checkout of the reference; its package `simulation` is imported from there).

    python tools/simmc_time.py [--ref DIR] [--cpu-only | --gpu-only] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_ISO, FS = 160000, 16000
ARRAY = np.array([[0.0425 * np.cos(a), 0.0425 * np.sin(a), 0.0] for a in np.arange(6) * np.pi / 3] + [[0.0, 0.0, 0.0]])


def device_median(fn, runs=10, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def gpu_lines():
    import torch
    from pykaldi2_amd import simulation
    import simmc_ref as R
    lines = []
    med, lo, hi = device_median(lambda: simulation.generate_isotropic_noise(ARRAY, N_ISO, FS, "sph", "hoth", seed=1))
    lines.append("generate_isotropic_noise 7 mics N=%d sph hoth (FFT 2^18): median %.3f ms (min %.3f, max %.3f) of 10" % (N_ISO, med, lo, hi))
    for part, fn in (("pk2_iso_spectra", lambda: simulation.iso_noise_spectra(ARRAY, N_ISO, FS, "sph", "hoth", seed=1)),):
        med, lo, hi = device_median(fn)
        lines.append("  of which %s: median %.3f ms (min %.3f, max %.3f)" % (part, med, lo, hi))
    X = simulation.iso_noise_spectra(ARRAY, N_ISO, FS, "sph", "hoth", seed=1)
    med, lo, hi = device_median(lambda: simulation.irfft_pow2(X))
    lines.append("  of which pk2_irfft_pow2_f32 (7 x 2^18): median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi))
    rs = np.random.RandomState(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    wavs = [dev(R.make_wav(rs, n, 0.3)) for n in (160000, 120000)]
    noises = [dev(R.make_wav(rs, n, 0.2)) for n in (60000, 200000)]
    rirs = [dev(R.make_rir(rs, 8000, 40 + 5 * i, 7)) for i in range(4)]
    delays = [40, 45, 50, 55]
    iso = simulation.generate_isotropic_noise(ARRAY, 64000, FS, "sph", "hoth", seed=2)
    sim = simulation.MultiSourceSimulator(array_geometry=ARRAY.T)
    np.random.seed(0)
    med, lo, hi = device_median(lambda: sim(wavs, noises, rirs[:2], rirs[2:], iso, get_early_reverb=True, rir_delays=delays))
    lines.append("MultiSourceSimulator 2 sources (10 s, 7.5 s) x 7 channels, 2 noises, 8000-tap RIRs, isotropic noise, early "
                 "reverberation: median %.3f ms (min %.3f, max %.3f) of 10" % (med, lo, hi))
    return lines


def cpu_lines(ref):
    import simmc_ref as R
    lines = []
    if ref:
        np.int = int
        sys.path.insert(0, ref)
        from simulation._iso_noise_simulator import generate_isotropic_noise
        np.random.seed(1)
        t = time.perf_counter()
        generate_isotropic_noise(ARRAY, N_ISO, FS, type="sph", spectrum="hoth")
        lines.append("reference generate_isotropic_noise, same call, numpy on the CPU: %.2f s (one run)" % (time.perf_counter() - t))
    else:
        t = time.perf_counter()
        R.iso_noise(ARRAY, N_ISO, FS, "sph", "hoth", R.legacy_draws(1, (1 << 18) // 2 + 1))
        lines.append("numpy restatement (tests/simmc_ref.py) of the same call on the CPU: %.2f s (one run)" % (time.perf_counter() - t))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="checkout of the reference: time its own generate_isotropic_noise")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simmc_time.txt"))
    args = ap.parse_args()
    lines = [] if args.cpu_only else gpu_lines()
    if not args.gpu_only:
        lines += cpu_lines(args.ref)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
