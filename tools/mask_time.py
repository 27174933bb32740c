"""Device time of the STFT, the inverse STFT and the ideal masks, written to profiles/mask_time.txt:

  * the masks of a 10 s two-source mixture: MaskEstimator on two clean signals against one distorted one (one STFT
    launch for the three signals, the clean masks' cutoffs, one mask launch), default analyzer (512 / 400 / 160, dither)
  * analyze and synthesize alone, one 10 s signal

each the median of 10 runs between device events after 2 warm-up runs, and next to them the CPU time of the same calls
in numpy: the restatement tests/mask_ref.py, or the reference's own classes with --ref DIR (a checkout of the reference;
its package `simulation` is imported from there).

    python tools/mask_time.py [--ref DIR] [--cpu-only | --gpu-only] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 160000


def signals():
    import mask_ref as R
    c0, d = R.inputs(1, N, 5)
    c1 = R.inputs(2, N, 5)[0]
    return c0, c1, (d + c1).astype(np.float32)


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
    c0, c1, d = [torch.from_numpy(x).cuda() for x in signals()]
    clean = torch.stack([c0, c1])
    an = simulation.SpectrumAnalyzer()
    est = simulation.MaskEstimator(an)
    lines = []
    med, lo, hi = device_median(lambda: est.get_mask_from_parallel_data(clean, d, seed=1))
    lines.append("MaskEstimator, 2 sources against one 10 s mixture (3 x %d samples, 1000 frames x 257 bins, dither): "
                 "median %.3f ms (min %.3f, max %.3f) of 10" % (N, med, lo, hi))
    med, lo, hi = device_median(lambda: an.analyze(c0, seed=1))
    lines.append("SpectrumAnalyzer.analyze, one 10 s signal, dither from the generator: median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi))
    quiet = simulation.SpectrumAnalyzer(do_dither=False)
    med, lo, hi = device_median(lambda: quiet.analyze(c0))
    lines.append("SpectrumAnalyzer.analyze, the same without dither: median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi))
    X = quiet.analyze(c0)
    med, lo, hi = device_median(lambda: quiet.synthesize(X))
    lines.append("SpectrumAnalyzer.synthesize of that spectrum (1000 frames): median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi))
    return lines


def cpu_lines(ref):
    import mask_ref as R
    c0, c1, d = signals()
    lines = []
    if ref:
        np.int = int
        sys.path.insert(0, ref)
        from simulation.freq_analysis import SpectrumAnalyzer
        from simulation.mask import MaskEstimator
        an = SpectrumAnalyzer()
        est = MaskEstimator(an)
        np.random.seed(1)
        t = time.perf_counter()
        for c in (c0, c1):
            est.get_mask_from_parallel_data(c, d)
        lines.append("reference MaskEstimator, the same two masks, numpy on the CPU: %.1f ms (one run)" % (1e3 * (time.perf_counter() - t)))
        t = time.perf_counter()
        X = an.analyze(c0)
        lines.append("reference SpectrumAnalyzer.analyze, one 10 s signal: %.1f ms (one run)" % (1e3 * (time.perf_counter() - t)))
        t = time.perf_counter()
        an.synthesize(X)
        lines.append("reference SpectrumAnalyzer.synthesize of that spectrum: %.1f ms (one run)" % (1e3 * (time.perf_counter() - t)))
    else:
        t = time.perf_counter()
        for c in (c0, c1):
            R.mask(c, d)
        lines.append("numpy restatement (tests/mask_ref.py) of the same two masks on the CPU, float64: %.1f ms (one run)"
                     % (1e3 * (time.perf_counter() - t)))
        t = time.perf_counter()
        X = R.stft(c0)
        lines.append("numpy restatement of analyze, one 10 s signal: %.1f ms (one run)" % (1e3 * (time.perf_counter() - t)))
        t = time.perf_counter()
        R.istft(X)
        lines.append("numpy restatement of synthesize: %.1f ms (one run)" % (1e3 * (time.perf_counter() - t)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="checkout of the reference: time its own SpectrumAnalyzer / MaskEstimator")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_time.txt"))
    args = ap.parse_args()
    lines = [] if args.cpu_only else gpu_lines()
    if not args.gpu_only:
        lines += cpu_lines(args.ref)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
