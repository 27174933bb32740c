"""Device time of MBR system combination, written to profiles/combine_time.txt: the 8 utterances of
tools/score_time.py decoded at two beams (two "systems") x the 33 settings of the recipes' sweep.  From one job:
`pk2_wordlat_combine` for max_iter = 1, 2, ... (the differences are the cost of each round: one E-step launch over every
system's lattice and one update launch) and for max_iter = 10 as a user calls it; `pk2_wordlat_best_path` and
`pk2_wordlat_mbr` with decode_mbr=0 on each system alone, whose difference -- one E-step of that system with its top entries
and decision -- is the yardstick a round is held against; the E-step counts.  Device time between events around the C ABI's
launches on buffers allocated once, median (min .. max) of 10 runs after 2 warm-ups.

    python tools/combine_time.py [--out FILE]
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

BEAMS = ((13.0, 6.0), (11.0, 4.0))


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


class Outputs:
    """The output buffers of pk2_wordlat_mbr / pk2_wordlat_combine for n pairs, allocated once."""

    def __init__(self, n, stride, dev):
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
        self.words, self.nw, self.status, self.iters, self.system = i32(n * stride), i32(n), i32(n), i32(n), i32(n)
        self.conf, self.risk, self.aend = f64(n * stride), f64(n), f64(n)
        self.stride = stride


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_time.txt"))
    args = ap.parse_args()
    lib, L = score._lib, score._lib.lib()
    settings = score.sweep()
    st, G = score._settings_array(settings), len(settings)
    systems = []
    for beam, lattice_beam in BEAMS:
        lens, dets = lattices(beam=beam, lattice_beam=lattice_beam)
        systems.append([score.pack_lattice(d, "%d@%g" % (n, beam)) for n, d in enumerate(dets)])
    N = len(systems[0])
    cb = score.CombinedBatch(systems)
    dev = cb.device
    lines = ["MBR system combination, %d utterances x %d systems x %d settings (tools/combine_time.py)" % (N, len(systems), G),
             "frames: %s" % lens]
    for (beam, lattice_beam), ps in zip(BEAMS, systems):
        lines.append("beam %g / %g, states / arcs / words / depth: " % (beam, lattice_beam) +
                     ", ".join("%d/%d/%d/%d" % (p.S, p.A, p.W, p.depth) for p in ps))
    lines.append("union vocabularies: %s words; capacities %s" % ([int(v.size) for v in cb.host["vocab"]], cb.host["cap"]))
    res = cb.mbr(settings)
    its = np.asarray([[r["iterations"] for r in row] for row in res])
    lines.append("combination, E-steps per pair: min %d, median %d, max %d; pairs still running in round 1, 2, ..: %s; "
                 "status counts %s; started from system 0 / 1: %s" % (
                     its.min(), int(np.median(its)), its.max(), [int((its >= k).sum()) for k in range(1, its.max() + 1)],
                     np.bincount([r["status"] for row in res for r in row], minlength=4).tolist(),
                     np.bincount([r["system"] for row in res for r in row], minlength=2).tolist()))
    # ---- each system alone: the yardstick ----
    yard = []
    for k, ps in enumerate(systems):
        batch = score.WordLatticeBatch(ps)
        own = batch.mbr(settings)
        oi = np.asarray([[r["iterations"] for r in row] for row in own])
        nbytes = int(L.pk2_wordlat_workspace_bytes(batch._h, 0, N, G, 0))
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        o = Outputs(N * G, max(p.depth for p in ps), dev)

        def best():
            lib.check(L.pk2_wordlat_best_path(batch._h, 0, N, lib.ptr(st), G, lib.ptr(work), nbytes, lib.ptr(o.words), o.stride,
                                              lib.ptr(o.nw), lib.ptr(o.risk), lib.ptr(o.aend), None, None, lib.ptr(o.status),
                                              lib.stream_ptr(dev)))

        def mbr(decode_mbr):
            lib.check(L.pk2_wordlat_mbr(batch._h, 0, N, lib.ptr(st), G, decode_mbr, 10, 0, lib.ptr(work), nbytes, lib.ptr(o.words),
                                        lib.ptr(o.conf), o.stride, lib.ptr(o.nw), lib.ptr(o.risk), lib.ptr(o.iters),
                                        lib.ptr(o.status), None, None, None, 0, lib.stream_ptr(dev)))
        tb, sb = timed(best)
        t1, s1 = timed(lambda: mbr(0))
        ta, sa = timed(lambda: mbr(1))
        yard.append(t1 - tb)
        lines.append("system %d alone (%d pairs), E-steps per pair min %d, median %d, max %d" % (k, N * G, oi.min(), int(np.median(oi)), oi.max()))
        lines.append("  pk2_wordlat_best_path                      %s" % sb)
        lines.append("  pk2_wordlat_mbr, decode_mbr=0 (one E-step)  %s   -> one E-step with its decision: %.4f ms" % (s1, t1 - tb))
        lines.append("  pk2_wordlat_mbr (all E-steps)               %s" % sa)
        del batch, work
    # ---- the combination ----
    nbytes = int(L.pk2_wordlat_combine_workspace_bytes(cb.batch._h, 0, N, G, 0))
    lines.append("workspace of the combination: %.2f MB" % (nbytes / 2 ** 20))
    work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    o = Outputs(N * G, max(1, max((c - 1) // 2 for c in cb.host["cap"])), dev)

    def combine(max_iter):
        lib.check(L.pk2_wordlat_combine(cb.batch._h, 0, N, lib.ptr(st), G, 1, max_iter, 0, lib.ptr(work), nbytes, lib.ptr(o.words),
                                        lib.ptr(o.conf), o.stride, lib.ptr(o.nw), lib.ptr(o.risk), lib.ptr(o.iters),
                                        lib.ptr(o.status), lib.ptr(o.system), None, None, None, 0, lib.stream_ptr(dev)))
    bb = score.WordLatticeBatch([p for g in cb.groups for p in g])
    pbytes = int(L.pk2_wordlat_workspace_bytes(bb._h, 0, len(bb), G, -1))
    ob = Outputs(len(bb) * G, max(p.depth for p in bb.packed), dev)
    tp, sp = timed(lambda: lib.check(L.pk2_wordlat_best_path(
        bb._h, 0, len(bb), lib.ptr(st), G, lib.ptr(work), pbytes, lib.ptr(ob.words), ob.stride, lib.ptr(ob.nw), lib.ptr(ob.risk),
        lib.ptr(ob.aend), None, None, lib.ptr(ob.status), lib.stream_ptr(dev))))
    lines.append("pk2_wordlat_best_path over both systems' lattices (what the combination starts with)  %s" % sp)
    prev, slow = tp, max(yard)
    for k in range(1, int(its.max()) + 1):
        t, s = timed(lambda: combine(k))
        lines.append("pk2_wordlat_combine, max_iter=%d  %s   -> round %d: %.4f ms = %.2f x the slower system's E-step (%.4f ms)"
                     % (k, s, k, t - prev, (t - prev) / slow, slow))
        prev = t
    t, s = timed(lambda: combine(10))
    lines.append("pk2_wordlat_combine, max_iter=10 (as called; the rounds after the last pair is done return at once)  %s" % s)
    lines.append("  -> the %d empty rounds: %.4f ms" % (10 - its.max(), t - prev))
    lines.append("expected before the run (DESIGN.md 7.17): round 1 = 1.0 to 1.15 x the slower system's E-step; the call 65 to 100 ms")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
