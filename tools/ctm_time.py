"""Device time of the word times of lattice scoring, written to profiles/ctm_time.txt: `pk2_wordlat_mbr` and
`pk2_wordlat_mbr_times` in the same job on the lattices of tools/score_time.py (8 determinised lattices of the synthetic
decoder x the 33 settings of the recipes' sweep), device time between events around the C ABI calls, buffers allocated once,
median (min .. max) of 10 runs after 2 warm-ups.  The difference of the two is what the times cost; next to it one E-step
of the batch (decode_mbr=False minus best_path) for scale, and what DESIGN.md expected before the run.

    python tools/ctm_time.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from score_time import lattices  # noqa: E402
from pykaldi2_amd import score  # noqa: E402


def timed(fn, runs=10, warm=2):
    ts = []
    for i in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), "%.4f ms (%.4f .. %.4f)" % (float(np.median(ts)), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctm_time.txt"))
    args = ap.parse_args()
    lens, dets = lattices()
    packed = [score.pack_lattice(d, str(n)) for n, d in enumerate(dets)]
    batch = score.WordLatticeBatch(packed)
    settings = score.sweep()
    L, lib, N, G = score._lib.lib(), score._lib, len(packed), len(settings)
    lines = ["word times of lattice scoring, %d determinised lattices x %d settings (tools/ctm_time.py)" % (N, G),
             "frames: %s" % lens,
             "states / arcs / words / depth: " + ", ".join("%d/%d/%d/%d" % (p.S, p.A, p.W, p.depth) for p in packed)]
    res = batch.mbr(settings, bins=2, times=True)            # computes and uploads the state times
    assert [int(t[-1]) for t in batch.state_time] == lens
    plain = batch.mbr(settings, bins=2)
    same = all(a["words"] == b["words"] and a["risk"] == b["risk"] and np.array_equal(a["conf"], b["conf"]) and a["bins"] == b["bins"]
               for ra, rb in zip(res, plain) for a, b in zip(ra, rb))
    its = [r["iterations"] for row in res for r in row]
    nw = [len(r["words"]) for row in res for r in row]
    lines.append("E-steps per pair: min %d, median %d, max %d; words per hypothesis: min %d, median %d, max %d; records with "
                 "times bit-identical to those without: %s" % (min(its), int(np.median(its)), max(its), min(nw),
                                                               int(np.median(nw)), max(nw), same))
    for bins in (0, 2):
        st = score._settings_array(settings)
        nb_mbr = int(L.pk2_wordlat_workspace_bytes(batch._h, 0, N, G, bins))
        nb = int(L.pk2_wordlat_times_workspace_bytes(batch._h, 0, N, G, bins))
        dev = batch.device
        work = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
        stride, bstride, n = max(p.depth for p in packed), max(p.cap for p in packed), N * G
        wi, wn, st_, it, bn = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n * stride, n, n, n, n))
        cf, rk, ae = (torch.empty(k, dtype=torch.float64, device=dev) for k in (n * stride, n, n))
        bw = torch.empty(max(1, n * bstride * bins), dtype=torch.int32, device=dev)
        bv = torch.empty(max(1, n * bstride * bins), dtype=torch.float64, device=dev)
        tm = torch.empty(n * stride * 2, dtype=torch.float64, device=dev)
        bt = torch.empty(max(1, n * bstride * bins * 2), dtype=torch.float64, device=dev)
        pt = torch.empty(n * stride * 2, dtype=torch.int32, device=dev)
        common = lambda dm, nbytes: (batch._h, 0, N, lib.ptr(st), G, dm, 10, bins, lib.ptr(work), nbytes, lib.ptr(wi), lib.ptr(cf),
                                     stride, lib.ptr(wn), lib.ptr(rk), lib.ptr(it), lib.ptr(st_), lib.ptr(bn), lib.ptr(bw),
                                     lib.ptr(bv), bstride)

        def best():
            lib.check(L.pk2_wordlat_best_path(batch._h, 0, N, lib.ptr(st), G, lib.ptr(work), nb, lib.ptr(wi), stride, lib.ptr(wn),
                                              lib.ptr(rk), lib.ptr(ae), None, None, lib.ptr(st_), lib.stream_ptr(dev)))

        def mbr(dm):
            lib.check(L.pk2_wordlat_mbr(*common(dm, nb_mbr), lib.stream_ptr(dev)))

        def mbr_times(dm):
            lib.check(L.pk2_wordlat_mbr_times(*common(dm, nb), lib.ptr(tm), lib.ptr(bt), lib.ptr(pt), stride, lib.stream_ptr(dev)))
        lines.append("bins = %d: workspace mbr %.2f MB, with times %.2f MB" % (bins, nb_mbr / 2 ** 20, nb / 2 ** 20))
        tb, sb = timed(best)
        t0, s0 = timed(lambda: mbr(1))
        t1, s1 = timed(lambda: mbr_times(1))
        e0, se0 = timed(lambda: mbr(0))
        e1, se1 = timed(lambda: mbr_times(0))
        lines += ["  best_path (pk2_wordlat_best_path)                        %s" % sb,
                  "  mbr (pk2_wordlat_mbr: posteriors + all E-steps)          %s" % s0,
                  "  mbr_times (pk2_wordlat_mbr_times: the same + the times)  %s" % s1,
                  "  mbr, decode_mbr=False (posteriors + one E-step)          %s" % se0,
                  "  mbr_times, decode_mbr=False                              %s" % se1,
                  "  the times cost %.4f ms (ratio %.4f) with decode_mbr, %.4f ms (ratio %.4f) without; one E-step of the batch "
                  "(decode_mbr=False minus best_path): %.4f ms" % (t1 - t0, t1 / t0, e1 - e0, e1 / e0, e0 - tb)]
    lines.append("expected before the run (DESIGN.md 7.15): the times cost 2 to 6 ms, a tenth to a third of one E-step of the batch")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
