"""Device time of lattice scoring, written to profiles/score_time.txt: `best_path` and `mbr` for 8
determinised lattices of the synthetic decoder x the 33 settings of the recipes' sweep, device time between events, median
(min .. max) of 10 runs after 2 warm-ups (the C ABI's launches alone, on buffers allocated once; `WordLatticeBatch.mbr` with its
allocations and the read-back of the results is timed on the host next to it).  Next to it, for orientation only: the numpy restatement's time for ONE (lattice, setting) pair on
this host, and what DESIGN.md expected before the run.

    python tools/score_time.py [--out FILE]
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
import mbr_ref  # noqa: E402
from pykaldi2_amd import lattice, score, synth  # noqa: E402


def lattices(num=8, P=120, words=200, seed=5, beam=13.0, lattice_beam=6.0):
    g = synth.decoding_graph_arcs(words, P, seed=seed, max_phones=3)
    tm = synth.transition_model_arrays(P)
    rec = lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(tm), g, 0.1,
                                                lattice.LatticeFasterDecoderOptions(beam=beam, lattice_beam=lattice_beam))
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(150, 400, num)]
    ll = np.zeros((num, max(lens), P), np.float32)
    for n, T in enumerate(lens):
        ll[n, :T] = 2.0 * rng.standard_normal((T, P))
    lat = rec.decode_batch(torch.from_numpy(ll).cuda(), lens)
    return lens, [lat.compact_lattice(n, determinize=True) for n in range(num)]


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
    return "%.4f ms (%.4f .. %.4f)" % (float(np.median(ts)), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_time.txt"))
    args = ap.parse_args()
    lens, dets = lattices()
    packed = [score.pack_lattice(d, str(n)) for n, d in enumerate(dets)]
    batch = score.WordLatticeBatch(packed)
    settings = score.sweep()
    lines = ["lattice scoring, %d determinised lattices x %d settings (tools/score_time.py)" % (len(packed), len(settings)),
             "frames: %s" % lens,
             "states / arcs / words / depth: " + ", ".join("%d/%d/%d/%d" % (p.S, p.A, p.W, p.depth) for p in packed),
             "workspace: best_path %.2f MB, mbr %.2f MB" % (
                 score._lib.lib().pk2_wordlat_workspace_bytes(batch._h, 0, len(packed), len(settings), -1) / 2 ** 20,
                 score._lib.lib().pk2_wordlat_workspace_bytes(batch._h, 0, len(packed), len(settings), 0) / 2 ** 20)]
    res = batch.mbr(settings)
    its = [r["iterations"] for row in res for r in row]
    lines.append("E-steps per pair: min %d, median %d, max %d; status counts %s" % (
        min(its), int(np.median(its)), max(its), np.bincount([r["status"] for row in res for r in row], minlength=4).tolist()))
    L, lib, N, G = score._lib.lib(), score._lib, len(packed), len(settings)
    st = score._settings_array(settings)
    nbytes = int(L.pk2_wordlat_workspace_bytes(batch._h, 0, N, G, 0))
    dev = batch.device
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    stride, n = max(p.depth for p in packed), N * G
    wi, wn, st_ = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n * stride, n, n))
    it = torch.empty(n, dtype=torch.int32, device=dev)
    cf, rk, ae = (torch.empty(k, dtype=torch.float64, device=dev) for k in (n * stride, n, n))

    def best():
        lib.check(L.pk2_wordlat_best_path(batch._h, 0, N, lib.ptr(st), G, lib.ptr(work), nbytes, lib.ptr(wi), stride, lib.ptr(wn),
                                          lib.ptr(rk), lib.ptr(ae), None, None, lib.ptr(st_), lib.stream_ptr(dev)))

    def mbr(decode_mbr):
        lib.check(L.pk2_wordlat_mbr(batch._h, 0, N, lib.ptr(st), G, decode_mbr, 10, 0, lib.ptr(work), nbytes, lib.ptr(wi),
                                    lib.ptr(cf), stride, lib.ptr(wn), lib.ptr(rk), lib.ptr(it), lib.ptr(st_), None, None, None, 0,
                                    lib.stream_ptr(dev)))
    lines.append("best_path (pk2_wordlat_best_path)  %s" % timed(best))
    lines.append("mbr (pk2_wordlat_mbr: posteriors + all E-steps)  %s" % timed(lambda: mbr(1)))
    lines.append("mbr, decode_mbr=False (posteriors + one E-step)  %s" % timed(lambda: mbr(0)))
    t0 = time.perf_counter()
    batch.mbr(settings)
    lines.append("WordLatticeBatch.mbr with allocations and read-back, host clock: %.2f ms" % (1e3 * (time.perf_counter() - t0)))
    big = int(np.argmax([p.A for p in packed]))
    t0 = time.perf_counter()
    mbr_ref.mbr(packed[big], settings[0])
    lines.append("numpy restatement, one pair (lattice %d, setting %s) on this host, for orientation: %.1f ms" % (
        big, settings[0][3], 1e3 * (time.perf_counter() - t0)))
    lines.append("expected before the run (DESIGN.md 7.13): mbr 1 to 2 ms, best_path 0.05 to 0.15 ms")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
