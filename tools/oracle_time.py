"""Device time of the lattice oracle, written to profiles/oracle_time.txt: `pk2_wordlat_oracle` on the 8
determinised lattices of tools/score_time.py (the ones tools/ctm_time.py uses) against (a) the decoder's one-best of every
utterance as its transcript and (b) those transcripts padded with words of the vocabulary to 63 / 64 / 200 words (one lane
chunk, two, four), with `pk2_wordlat_best_path` for ONE setting in the same job for scale.  Device time between events
around windows of 20 C ABI calls on buffers allocated once, per call: median (min .. max) of 10 windows after 2 warm-up
windows.  Next to it the host time of `WordLatticeBatch.oracle` (allocations, uploads and read-back included) and the time
of the restatement tests/oracle_ref.py on the largest lattice -- the only other way to the number -- and what DESIGN.md
expected before the run.

    python tools/oracle_time.py [--out FILE]
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
import oracle_ref  # noqa: E402
from score_time import lattices  # noqa: E402
from pykaldi2_amd import score  # noqa: E402

EXPECTED = {"transcripts": "0.2 to 0.6 ms", "63": "0.5 to 1.5 ms", "64": "1 to 2 ms", "200": "1.5 to 4 ms"}


def timed(fn, windows=10, warm=2, reps=20):
    ts = []
    for i in range(warm + windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts)), "%.4f ms (%.4f .. %.4f)" % (float(np.median(ts)), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oracle_time.txt"))
    args = ap.parse_args()
    lens, dets = lattices()
    packed = [score.pack_lattice(d, str(n)) for n, d in enumerate(dets)]
    batch = score.WordLatticeBatch(packed)
    L, lib, N, dev = score._lib.lib(), score._lib, len(packed), batch.device
    rng = np.random.default_rng(0)
    base = [[int(w) for w in d["best_words"]] for d in dets]
    pad = lambda r, n, P: (r + [int(w) for w in rng.choice(P.word_ids[1:], n)])[:n]
    cases = [("transcripts", base)] + [(str(n), [pad(r, n, P) for r, P in zip(base, packed)]) for n in (63, 64, 200)]
    depth = [score.lattice_depth(P) for P in packed]
    lines = ["lattice oracle, %d determinised lattices (tools/oracle_time.py)" % N, "frames: %s" % lens,
             "states / arcs / words / depth: " + ", ".join("%d/%d/%d/%d" % (p.S, p.A, p.W, p.depth) for p in packed),
             "lattice depth (arc-frames / frames): " + ", ".join("%.2f" % (a / t) for a, t in depth) +
             "; all: %.2f" % (sum(a for a, _ in depth) / sum(t for _, t in depth))]
    labels = batch._arc_labels(())
    stride = max(p.depth for p in packed)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    errors, counts, status, nw, npath, words, path = i32(N), i32(3 * N), i32(N), i32(N), i32(N), i32(N * stride), i32(N * stride)
    big = int(np.argmax([p.S for p in packed]))
    for name, refs in cases:
        recs = batch.oracle(refs)
        want = oracle_ref.oracle(packed[big], refs[big])
        same = all(recs[big][f] == want[f] for f in ("errors", "ins", "dele", "sub", "words", "arcs"))
        local = [oracle_ref.local_ref(P, r).astype(np.int32) for P, r in zip(packed, refs)]
        off = np.concatenate([[0], np.cumsum([r.size for r in local])]).astype(np.int64)
        ref_dev, off_dev = lib.h2d(np.ascontiguousarray(np.concatenate(local)), dev), lib.h2d(off, dev)
        nb = int(L.pk2_wordlat_oracle_workspace_bytes(batch._h, 0, N, lib.ptr(off)))
        work = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)

        def call():
            lib.check(L.pk2_wordlat_oracle(batch._h, 0, N, lib.ptr(labels), lib.ptr(ref_dev), lib.ptr(off_dev), lib.ptr(off),
                                           lib.ptr(work), nb, lib.ptr(errors), lib.ptr(counts), lib.ptr(words), stride,
                                           lib.ptr(nw), lib.ptr(path), stride, lib.ptr(npath), lib.ptr(status),
                                           lib.stream_ptr(dev)))
        _, s = timed(call)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            batch.oracle(refs)
        host = (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        oracle_ref.oracle(packed[big], refs[big])
        tref = time.perf_counter() - t0
        cells = sum(p.S * (len(r) + 1) for p, r in zip(packed, refs))
        loads = sum(2 * p.A * (len(r) + 1) for p, r in zip(packed, refs))
        lines += ["references: %s (words per reference %s); errors %s of %d reference words, ins / del / sub %d / %d / %d"
                  % (name, [len(r) for r in refs], [r["errors"] for r in recs], sum(len(r) for r in refs),
                     sum(r["ins"] for r in recs), sum(r["dele"] for r in recs), sum(r["sub"] for r in recs)),
                  "  table cells %d, row loads %d (%.1f MB), workspace %.2f MB; largest lattice equal to the restatement: %s"
                  % (cells, loads, 4e-6 * loads, nb / 2 ** 20, same),
                  "  pk2_wordlat_oracle, the batch                     %s   expected before the run: %s" % (s, EXPECTED[name]),
                  "  WordLatticeBatch.oracle on the host clock         %.3f ms" % (1e3 * host),
                  "  tests/oracle_ref.py, the largest lattice alone    %.1f ms on this host's CPU" % (1e3 * tref)]
    st = score._settings_array(score.sweep()[:1])
    nb = int(L.pk2_wordlat_workspace_bytes(batch._h, 0, N, 1, -1))
    work = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    cost, ae = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(2))

    def best():
        lib.check(L.pk2_wordlat_best_path(batch._h, 0, N, lib.ptr(st), 1, lib.ptr(work), nb, lib.ptr(words), stride, lib.ptr(nw),
                                          lib.ptr(cost), lib.ptr(ae), None, None, lib.ptr(status), lib.stream_ptr(dev)))
    lines.append("for scale: pk2_wordlat_best_path, the batch x 1 setting  %s" % timed(best)[1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
