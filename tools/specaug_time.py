"""Device time of SpecAugment, written to profiles/specaug_time.txt, on the four frame counts of the LF-MMI
benchmark's first minibatch (synth.utterance_durations of generator 1234) with the default masks and time_warp 40:

  (a) masks in place                      pk2_spec_augment, has_warp = 0, in == out: only the masked elements are written
  (b) warp plus masks, out of place       pk2_spec_augment, has_warp = 1: every row is read (two rows where it interpolates)
  the yardstick: feats.clone() of the same tensor in the same run -- a copy moves what (b) must move

each the median of 10 runs between device events after 2 warm-up runs, for the launch alone (plan already on the device) and
for augment.spec_augment as the trainers call it (plan check on the host, pinned upload, launch).

    python tools/specaug_time.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return "median %.4f ms (min %.4f, max %.4f) of %d" % (float(np.median(times)), min(times), max(times), runs)


def lines():
    import torch
    from pykaldi2_amd import _lib, augment, fbank, synth
    frames = [fbank.num_frames(int(round(16000 * d))) for d in synth.utterance_durations(np.random.default_rng(1234), 4)]
    total = sum(frames)
    feats = torch.from_numpy(np.random.default_rng(0).standard_normal((total, 80)).astype(np.float32)).cuda()
    out = torch.empty_like(feats)
    off = np.zeros(len(frames) + 1, np.int64)
    off[1:] = np.cumsum(frames)
    row_off = torch.from_numpy(off).cuda()
    aug = augment.SpecAugment(time_warp=40)
    plan = aug.draw(aug.generator(0, 0), frames)
    masks = plan.copy()
    masks[:, :2] = 0
    plan_dev, masks_dev = torch.from_numpy(plan).cuda(), torch.from_numpy(masks).cuda()
    call, stream = _lib.lib().pk2_spec_augment, _lib.stream_ptr(feats.device)
    masked = int(sum(int((masks[n, 11::2] - masks[n, 10::2]).sum()) for n in range(len(frames))))      # an upper bound: overlaps

    def launch(dst, p, warp):
        _lib.check(call(_lib.ptr(feats), _lib.ptr(dst), _lib.ptr(row_off), len(frames), total, _lib.ptr(p), warp, 0.0, stream))
    res = ["frames %s = %d rows, %.2f MB; plan: time_warp 40, (c, d) %s, at most %d masked frames, bands %s"
           % (frames, total, total * 320 / 1e6, plan[:, :2].tolist(), masked, plan[:, 2:6].tolist()),
           "(a) masks in place, launch alone: %s" % device_median(lambda: launch(feats, masks_dev, 0)),
           "(a) masks in place, augment.spec_augment: %s" % device_median(lambda: augment.spec_augment(feats, row_off, frames, masks)),
           "(b) warp plus masks out of place, launch alone: %s" % device_median(lambda: launch(out, plan_dev, 1)),
           "(b) warp plus masks out of place, augment.spec_augment: %s"
           % device_median(lambda: augment.spec_augment(feats, row_off, frames, plan, out=out)),
           "masks out of place (no warp), launch alone: %s" % device_median(lambda: launch(out, masks_dev, 0)),
           "feats.clone() of the same tensor: %s" % device_median(lambda: feats.clone())]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specaug_time.txt"))
    args = ap.parse_args()
    res = lines()
    with open(args.out, "w") as f:
        f.write("\n".join(res) + "\n")
    print("\n".join(res))


if __name__ == "__main__":
    main()
