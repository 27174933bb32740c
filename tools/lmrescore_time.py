"""Device time of n-gram LM rescoring, written to profiles/lmrescore_time.txt: the 8 determinised lattices
of tools/score_time.py composed with a synthetic 3-gram LM over the 200 words of the loop, device time between events
around the C ABI's launch on buffers allocated once, median (min .. max) of 10 runs after 2 warm-ups; `score.rescore_lm`
with its packing, allocations and read-back on the host clock next to it.  For orientation only: the pure-Python
restatement's time for the largest lattice on this host, and what DESIGN.md expected before the run.

    python tools/lmrescore_time.py [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lmrescore_ref  # noqa: E402
from score_time import lattices, timed  # noqa: E402
from pykaldi2_amd import ngram, score  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmrescore_time.txt"))
    ap.add_argument("--expand", default=8.0, type=float)
    args = ap.parse_args()
    lens, dets = lattices()
    ngrams, bos, eos = lmrescore_ref.random_lm(200, 3, 7, density=0.1)
    lm = ngram.NgramLM.from_ngrams(ngrams, bos, eos, 3)
    batch = score.WordLatticeBatch(dets)
    packed, N, dev = batch.packed, len(dets), batch.device
    L, lib = score._lib.lib(), score._lib
    out = score.rescore_lm(dets, [(lm, 1.0)], expand=args.expand)
    lines = ["n-gram LM rescoring, %d determinised lattices (tools/lmrescore_time.py)" % N,
             "frames: %s" % lens,
             "LM: order 3, %d n-grams (%s per order), synthetic, 200 words" % (lm.num_nodes - 1, np.diff(lm.order_off)[1:].tolist()),
             "states / arcs / depth in: " + ", ".join("%d/%d/%d" % (p.S, p.A, p.depth) for p in packed),
             "states / arcs out: " + ", ".join("%d/%d" % (o["num_states"], o["src"].size) for o in out),
             "expansion (states, arcs): " + ", ".join("%.2f/%.2f" % (o["num_states"] / p.S, o["src"].size / p.A)
                                                      for o, p in zip(out, packed))]
    nbytes = int(L.pk2_wordlat_lmrescore_workspace_bytes(batch._h, 0, N, args.expand))
    nS, nA = sum(int(args.expand * p.S) for p in packed), sum(int(args.expand * p.A) for p in packed)
    lines.append("expand %g: workspace %.2f MB, output room %.2f MB" % (args.expand, nbytes / 2 ** 20, (8 * nS + 24 * nA) / 2 ** 20))
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    ons, ona, st = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    states, arcs = torch.empty(2 * nS, dtype=torch.int32, device=dev), torch.empty(6 * nA, dtype=torch.int32, device=dev)
    words = lib.h2d(score._lm_words(batch, lm), dev)
    h_lm = lm.handle(dev)

    def run():
        lib.check(L.pk2_wordlat_lmrescore(batch._h, 0, N, h_lm, lib.ptr(words), 1.0, args.expand, lib.ptr(work), nbytes, lib.ptr(ons),
                                          lib.ptr(ona), lib.ptr(states), nS, lib.ptr(arcs), nA, lib.ptr(st), lib.stream_ptr(dev)))
    lines.append("pk2_wordlat_lmrescore, one launch for the batch  %s" % timed(run))
    lines.append("status: %s" % st.cpu().tolist())
    t0 = time.perf_counter()
    score.rescore_lm(dets, [(lm, 1.0)], expand=args.expand)
    lines.append("score.rescore_lm with packing, allocations and read-back, host clock: %.2f ms" % (1e3 * (time.perf_counter() - t0)))
    big = int(np.argmax([p.A for p in packed]))
    ref = lmrescore_ref.RefLM(ngrams, bos, eos, 3)
    t0 = time.perf_counter()
    want = lmrescore_ref.compose(packed[big], ref, 1.0)
    lines.append("pure-Python restatement, lattice %d alone on this host, for orientation: %.1f ms" % (big, 1e3 * (time.perf_counter() - t0)))
    lines.append("device == restatement on lattice %d: %s" % (big, lmrescore_ref.same_composition(out[big], want) is None))
    lines.append("expected before the run (DESIGN.md 7.14): 4 to 8 ms per launch")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
