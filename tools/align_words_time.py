"""Device time of the word-boundary alignment, written to profiles/align_words_time.txt: `pk2_wordlat_best_path`
alone and `pk2_wordlat_best_path` + `pk2_wordlat_align_words` in the same job on the lattices of tools/score_time.py (8
determinised lattices of the synthetic decoder x the 33 settings of the recipes' sweep), device time between events around
the C ABI calls, buffers allocated once, median (min .. max) of 10 runs after 2 warm-ups.  Next to it the sequential
restatement (tests/align_words_ref.py) on the same 264 paths as host wall time, and what DESIGN.md expected before the run.

    python tools/align_words_time.py [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from score_time import lattices  # noqa: E402
from ctm_time import timed  # noqa: E402
import align_words_ref as A  # noqa: E402
from pykaldi2_amd import score, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_words_time.txt"))
    args = ap.parse_args()
    lens, dets = lattices()
    batch = score.WordLatticeBatch(dets)
    packed = batch.packed
    settings = score.sweep()
    tm = synth.transition_model_topology(120)
    wb = score.WordBoundary({p: "nonword" if p == 1 else "singleton" for p in range(1, 41)})
    L, lib, N, G = score._lib.lib(), score._lib, len(packed), len(settings)
    recs = batch.align_words(settings, tm, wb, phones=True)          # uploads the strings
    post = batch.arc_posteriors(settings)
    t0 = time.perf_counter()
    refs = [[A.align_ref(batch, n, post[n][g], tm, wb) for g in range(G)] for n in range(N)]
    host = time.perf_counter() - t0
    for ra, rb in zip(recs, refs):
        for a, b in zip(ra, rb):
            A.same_record(a, b)
    nph = [len(r["phones"]) for row in recs for r in row]
    nst = [r["status"] for row in recs for r in row]
    lines = ["word-boundary alignment, %d determinised lattices x %d settings (tools/align_words_time.py)" % (N, G),
             "frames: %s" % lens, "frame capacity: %s" % batch.frame_cap,
             "states / arcs / words / depth: " + ", ".join("%d/%d/%d/%d" % (p.S, p.A, p.W, p.depth) for p in packed),
             "phones per path: min %d, median %d, max %d; pairs with status 0: %d, 1: %d (the synthetic lexicon is not "
             "position-dependent); all %d records equal the restatement" % (min(nph), int(np.median(nph)), max(nph), nst.count(0),
                                                                            nst.count(1), N * G)]
    st = score._settings_array(settings)
    dev = batch.device
    nb = int(L.pk2_wordlat_workspace_bytes(batch._h, 0, N, G, -1))
    na = int(L.pk2_wordlat_align_workspace_bytes(batch._h, 0, N, G))
    work = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    awork = torch.empty(na // 8 + 1, dtype=torch.float64, device=dev)
    stride, fstride, n = max(p.depth for p in packed), max(batch.frame_cap), N * G
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
    wi, wn, bs, bp = i32(n * stride), i32(n), i32(n), i32(G * int(batch._host["state_off"][-1]))
    cost, ae = f64(n), f64(n)
    pt, wt, tok, ntok, pho, nphones, status, reason = (i32(n * stride * 2), i32(n * stride * 2), i32(n * fstride * 4), i32(n),
                                                      i32(n * fstride * 3), i32(n), i32(n), i32(n))
    model = batch._align_models[(id(tm), id(wb))]

    def best():
        lib.check(L.pk2_wordlat_best_path(batch._h, 0, N, lib.ptr(st), G, lib.ptr(work), nb, lib.ptr(wi), stride, lib.ptr(wn),
                                          lib.ptr(cost), lib.ptr(ae), None, lib.ptr(bp), lib.ptr(bs), lib.stream_ptr(dev)))

    def align(with_phones):
        lib.check(L.pk2_wordlat_align_words(batch._h, model.h, 0, N, G, lib.ptr(bp), lib.ptr(bs), lib.ptr(awork), na, lib.ptr(pt),
                                            lib.ptr(wt), stride, lib.ptr(tok), lib.ptr(ntok), fstride,
                                            lib.ptr(pho) if with_phones else None, lib.ptr(nphones), fstride, lib.ptr(status),
                                            lib.ptr(reason), lib.stream_ptr(dev)))

    def both(with_phones):
        best()
        align(with_phones)
    lines.append("workspace: best path %.2f MB, alignment %.2f MB" % (nb / 2 ** 20, na / 2 ** 20))
    tb, sb = timed(best)
    t1, s1 = timed(lambda: both(False))
    t2, s2 = timed(lambda: both(True))
    best()
    ta, sa = timed(lambda: align(False))
    lines += ["  best_path (pk2_wordlat_best_path, with back-pointers)         %s" % sb,
              "  best_path + align_words (pk2_wordlat_align_words)             %s" % s1,
              "  best_path + align_words with the phone rows                   %s" % s2,
              "  align_words alone, on the back-pointers left behind           %s" % sa,
              "  the alignment costs %.4f ms (ratio %.4f to the best path alone); the restatement on the same %d paths: %.1f ms of "
              "host wall time" % (t1 - tb, t1 / tb, N * G, 1e3 * host),
              "expected before the run (DESIGN.md 7.18): 0.02 to 0.06 ms for the alignment of the batch, one round of 264 "
              "workgroups bound by the latency of about 20 barrier-separated steps, not by traffic"]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
