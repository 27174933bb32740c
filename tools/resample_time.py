"""Device time of the resampler, written to profiles/resample_time.txt:

  * the four utterance lengths of the LF-MMI benchmark's first minibatch (synth.utterance_durations of generator 1234), each
    at a drawn speed factor of 0.9 / 1.0 / 1.1 with a volume gain: one launch (augment.speed_perturb)
  * 48000 -> 16000 of a 10 s signal
  * the coprime ratio 15217 -> 16000 of a 10 s signal (16000 phases: the weight table is read from memory), and
    14400 -> 16000 of the same signal with its weights in LDS and, PK2_RESAMPLE_WEIGHTS=mem, read from memory

each the median of 10 runs between device events after 2 warm-up runs, and next to each the host time of the float64
restatement tests/resample_ref.py on the same input (one run).

    python tools/resample_time.py [--cpu-only | --gpu-only] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases():
    from pykaldi2_amd import synth
    rng = np.random.default_rng(0)
    lens = [int(round(16000 * d)) for d in synth.utterance_durations(np.random.default_rng(1234), 4)]
    factors = [[0.9, 1.0, 1.1][int(i)] for i in np.random.default_rng(7).integers(3, size=4)]
    if all(f == 1.0 for f in factors):
        factors[0] = 0.9
    gains = [float(g) for g in np.random.default_rng(8).uniform(0.125, 2.0, size=4)]
    ratios = [(int(round(16000 * f)), 16000) for f in factors]
    mb = [rng.standard_normal(n).astype(np.float32) for n in lens]
    ten48 = rng.standard_normal(480000).astype(np.float32)
    ten = rng.standard_normal(152170).astype(np.float32)
    return [("bench minibatch %s samples at factors %s, gains folded in" % (lens, factors), mb, ratios, gains, None),
            ("48000 -> 16000, 10 s", [ten48], [(48000, 16000)], [1.0], None),
            ("15217 -> 16000 (coprime, 16000 phases), 10 s", [ten], [(15217, 16000)], [1.0], None),
            ("14400 -> 16000, %d samples, weights in LDS" % len(ten), [ten], [(14400, 16000)], [1.0], ""),
            ("14400 -> 16000, %d samples, weights from memory" % len(ten), [ten], [(14400, 16000)], [1.0], "mem")]


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
    from pykaldi2_amd import augment
    names = {augment.PATH_LDS: "LDS", augment.PATH_MEM: "memory", augment.PATH_LDS | augment.PATH_MEM: "LDS + memory"}
    lines = []
    for what, xs, ratios, gains, force in cases():
        wav = torch.from_numpy(np.concatenate(xs)).cuda()
        lens = [len(x) for x in xs]
        if force is not None:
            os.environ["PK2_RESAMPLE_WEIGHTS"] = force
        med, lo, hi = device_median(lambda: augment.resample_ragged(wav, lens, ratios, gains))
        os.environ.pop("PK2_RESAMPLE_WEIGHTS", None)
        lines.append("%s: median %.3f ms (min %.3f, max %.3f) of 10, weight path %s, %d samples in"
                     % (what, med, lo, hi, names.get(augment.last_path(), "?"), sum(lens)))
    return lines


def cpu_lines():
    import resample_ref as R
    lines = []
    for what, xs, ratios, gains, force in cases():
        if force == "mem":
            continue
        t = time.perf_counter()
        for x, r, g in zip(xs, ratios, gains):
            R.resample(x, r[0], r[1], g)
        lines.append("numpy restatement (tests/resample_ref.py), float64, %s: %.1f ms on the host (one run)"
                     % (what.split(" samples")[0].split(", 10 s")[0].split(", %d" % len(xs[0]))[0], 1e3 * (time.perf_counter() - t)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.txt"))
    args = ap.parse_args()
    lines = [] if args.cpu_only else gpu_lines()
    if not args.gpu_only:
        lines += cpu_lines()
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
