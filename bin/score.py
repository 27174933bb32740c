#!/usr/bin/env python
"""Scores a compact-lattice archive against reference transcripts -- the last step of the reference's recipes
(example/*/local/score*.sh: lattice-scale | lattice-add-penalty | lattice-best-path or lattice-mbr-decode for every LM
weight and word insertion penalty, then utt_wer.py), running on libpk2hip.so: every (lattice, setting) pair of a batch is
decoded in one launch (pykaldi2_amd.score), the word errors are counted on the device.

  python bin/score.py -lat_file exp/se/lat.ark -words_txt exp/tri/graph/words.txt -ref_text data/dev/text \
      -out_dir exp/se/scoring [-min_lmwt 7 -max_lmwt 17 -word_ins_penalty 0.0,0.5,1.0] [-decode_mbr] [-ctm -frame_shift 0.03] \
      [-oracle] [-combine exp/tf/lat.ark[,exp/x/lat.ark,...] [-lat_weights 0.6:0.4]] \
      [-ctm -word_boundary lang/phones/word_boundary.int -model exp/tri/final.mdl [-phone_ctm]]

Writes hyp_<LMWT>.<wip>.txt (key, then words) and result_<LMWT>_<wip> (utt_wer.py's three lines per utterance: reco:, ref:,
`<key> err: E ref_len: L`; with -decode_mbr a fourth line `conf: <key> c1 c2 ...`) per setting and prints
`best: LMWT=.. wip=.. errors=.. ref_words=.. WER=..%` last: the lowest error count, ties to the first setting of the sweep.
<NOISE> and <SPOKEN_NOISE> are removed from the references and <UNK> from the hypotheses (score_opencss.sh).  Lattices
without a reference are reported and skipped; a reference without a lattice counts all its words as errors.
-ctm adds ctm_<LMWT>_<wip> per setting (score_sclite.sh's lattice-to-ctm-conf): `<key> 1 <begin> <duration> <word> <confidence>`
in seconds, keys in archive order, the times of the lattice's own word arcs (-word_boundary aligns them) -- of the MBR
hypothesis with -decode_mbr, otherwise of the best path with its confidences (--decode-mbr=false).
-oracle adds what lattice-oracle and lattice-depth report: oracle.txt (key, then the words of the lattice path closest to the
reference), result_oracle (reco: / ref: / err: as above and `<key> ins: I del: D sub: S`) and, before the `best:` line,
`oracle: errors=E ref_words=N WER=x.xx% ins=I del=D sub=S depth=d.dd` -- the floor under every result_* file; <UNK> arcs
cost nothing, as <UNK> is dropped from the hypotheses; depth = arc-frames over frames of all lattices.
-combine adds the lattices that other systems made of the same utterances (score_combine.sh: lattice-combine
--lat-weights=w1:w2:.. | lattice-mbr-decode): every utterance of -lat_file is decoded by minimum Bayes risk over the weighted
union of its lattices (pykaldi2_amd.score.CombinedBatch; equal weights without -lat_weights, the first weight is -lat_file's).
A key that another archive lacks is reported and combined from the systems that have it.  The output files are those of
-decode_mbr; -ctm and -oracle are not available with it.
-word_boundary with -model (and -ctm, without -decode_mbr) is score_ctm.sh's lattice-1best | lattice-align-words | nbest-to-ctm:
the ctm_* files carry every word's own begin and end, found by cutting the best path's transition-id string into phones and
grouping them by word_boundary.int (pykaldi2_amd.score.WordLatticeBatch.align_words); the confidences stay as they are.  A
path whose string is not a sequence of whole words keeps its arcs' times; `aligned: P of Q pairs, fallback: F` counts them.
-phone_ctm adds phone_ctm_<LMWT>_<wip> (lattice-align-phones): `<key> 1 <begin> <duration> <phone-id>`.  An MBR or combined
hypothesis is not a path, so -word_boundary is refused with -decode_mbr and -combine."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import kaldi_io, lattice, score  # noqa: E402

REF_FILTER = ("<NOISE>", "<SPOKEN_NOISE>")
HYP_FILTER = ("<UNK>",)


def read_words_txt(path):
    table = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) == 2:
                table[int(parts[1])] = parts[0]
    return table


def read_text(path):
    refs = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if parts:
                refs[parts[0]] = [w for w in parts[1:] if w not in REF_FILTER]
    return refs


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("-lat_file", required=True, help="binary compact-lattice archive (bin/latgen.py -out_file)")
    parser.add_argument("-words_txt", required=True, help="the graph directory's words.txt")
    parser.add_argument("-ref_text", required=True, help="Kaldi text: key, then the reference words")
    parser.add_argument("-out_dir", required=True)
    parser.add_argument("-min_lmwt", default=7, type=int)
    parser.add_argument("-max_lmwt", default=17, type=int)
    parser.add_argument("-word_ins_penalty", default="0.0,0.5,1.0")
    parser.add_argument("-decode_mbr", action="store_true", help="minimum Bayes risk decoding with word confidences")
    parser.add_argument("-ctm", action="store_true", help="also write ctm_<LMWT>_<wip>: word times and confidences")
    parser.add_argument("-frame_shift", default=0.01, type=float, help="seconds per frame (0.03 for a chain model)")
    parser.add_argument("-oracle", action="store_true", help="also write oracle.txt / result_oracle: the lattice oracle WER")
    parser.add_argument("-combine", default="", help="comma-separated archives of further systems: MBR system combination")
    parser.add_argument("-lat_weights", default="", help="w1:w2:... for -lat_file and the archives of -combine (default: equal)")
    parser.add_argument("-word_boundary", default="", help="phones/word_boundary.int: align the CTM times to the words' own phones")
    parser.add_argument("-model", default="", help="final.mdl (or its text form), for -word_boundary")
    parser.add_argument("-phone_ctm", action="store_true", help="with -word_boundary: also write phone_ctm_<LMWT>_<wip>")
    parser.add_argument("-batch_size", default=32, type=int, help="lattices per device batch")
    args = parser.parse_args()
    others = [x for x in args.combine.split(",") if x.strip()]
    if args.word_boundary:
        if args.decode_mbr:
            parser.error("-word_boundary is not available with -decode_mbr: an MBR hypothesis is not a path of the lattice")
        if others:
            parser.error("-word_boundary is not available with -combine: a combined hypothesis is not a path of a lattice")
        if not args.model:
            parser.error("-word_boundary needs -model (final.mdl)")
        if not args.ctm:
            parser.error("-word_boundary needs -ctm")
    elif args.model or args.phone_ctm:
        parser.error("-model and -phone_ctm need -word_boundary")
    if others:
        for flag in ("ctm", "oracle"):
            if getattr(args, flag):
                parser.error("-%s is not available with -combine" % flag)
        args.decode_mbr = True
    elif args.lat_weights:
        parser.error("-lat_weights needs -combine")
    lat_weights = [float(x) for x in args.lat_weights.split(":") if x.strip()] or None
    if lat_weights is not None and len(lat_weights) != 1 + len(others):
        parser.error("-lat_weights: %d weights for %d systems" % (len(lat_weights), 1 + len(others)))

    boundary = score.WordBoundary.read(args.word_boundary) if args.word_boundary else None
    trans_model = lattice.TransitionModel.read(args.model) if args.word_boundary else None
    symbols = read_words_txt(args.words_txt)
    refs = read_text(args.ref_text)
    wips = [float(x) for x in args.word_ins_penalty.split(",") if x.strip()]
    settings = score.sweep(args.min_lmwt, args.max_lmwt, wips)
    G = len(settings)
    os.makedirs(args.out_dir, exist_ok=True)
    # word <-> integer for the error count: the symbol table's ids, new ids for reference words it does not hold
    ids = {s: i for i, s in symbols.items()}
    next_id = max(list(symbols) + [0]) + 1

    def word_id(w):
        nonlocal next_id
        if w not in ids:
            ids[w] = next_id
            next_id += 1
        return ids[w]

    hyps = [dict() for _ in range(G)]      # per setting: key -> (words, confidences)
    ctm = [dict() for _ in range(G)]       # per setting: key -> CTM lines
    phone_ctm = [dict() for _ in range(G)]  # per setting: key -> phone CTM lines (-phone_ctm)
    aligned = [0, 0, 0]                    # -word_boundary: pairs aligned, pairs, pairs that kept their arcs' times
    oracle = {}                            # key -> record of WordLatticeBatch.oracle
    depth = [0, 0]                         # arc-frames, frames over all lattices
    skip = [i for i, s in symbols.items() if s in HYP_FILTER]
    seen, batch, order = set(), [], []
    extra = [dict(kaldi_io.read_compact_lattice_ark(path)) for path in others]     # the other systems' lattices by key

    def flush():
        if not batch:
            return
        if others:
            for path, table in zip(others, extra):
                for key, _ in batch:
                    if key not in table:
                        print("no lattice for %s in %s: combined from the other systems" % (key, path))
            cb = score.CombinedBatch([[lat for _, lat in batch]] + [[table.get(k) for k, _ in batch] for table in extra], "cuda",
                                     names=[k for k, _ in batch], weights=lat_weights)
            for g0 in range(0, G, score.MAX_SETTINGS):
                for (key, _), row in zip(batch, cb.mbr(settings[g0:g0 + score.MAX_SETTINGS])):
                    for g, rec in enumerate(row):
                        keep = [i for i, w in enumerate(rec["words"]) if symbols.get(w, str(w)) not in HYP_FILTER]
                        hyps[g0 + g][key] = ([symbols.get(rec["words"][i], str(rec["words"][i])) for i in keep],
                                             [float(rec["conf"][i]) for i in keep])
            del batch[:]
            return
        wl = score.WordLatticeBatch([lat for _, lat in batch], "cuda", names=[k for k, _ in batch])
        for g0 in range(0, G, score.MAX_SETTINGS):
            part = settings[g0:g0 + score.MAX_SETTINGS]
            timed = wl.mbr(part, decode_mbr=args.decode_mbr, times=True) if args.ctm and boundary is None else None
            if args.decode_mbr:
                res = timed if args.ctm else wl.mbr(part, decode_mbr=True)
            else:
                res = [[dict(words=w, conf=None) for w, _ in row] for row in wl.best_path(part)]
            if boundary is not None:
                for (key, _), row, crow in zip(batch, wl.align_words(part, trans_model, boundary, phones=args.phone_ctm),
                                               wl.mbr(part, decode_mbr=False)):
                    for g, (rec, crec) in enumerate(zip(row, crow)):
                        conf = crec["conf"] if crec["words"] == rec["words"] else np.ones(len(rec["words"]))
                        ctm[g0 + g][key] = score.ctm_lines(key, dict(rec, conf=conf), symbols, args.frame_shift, drop=HYP_FILTER)
                        aligned[0] += rec["status"] == 0
                        aligned[1] += 1
                        aligned[2] += rec["status"] == 1
                        if args.phone_ctm:
                            phone_ctm[g0 + g][key] = ["%s 1 %.3f %.3f %d" % (key, b * args.frame_shift, d * args.frame_shift, p)
                                                      for p, b, d in rec["phones"].tolist()]
            elif args.ctm:
                for (key, _), row in zip(batch, timed):
                    for g, rec in enumerate(row):
                        ctm[g0 + g][key] = score.ctm_lines(key, rec, symbols, args.frame_shift, drop=HYP_FILTER)
            for (key, _), row in zip(batch, res):
                for g, rec in enumerate(row):
                    keep = [i for i, w in enumerate(rec["words"]) if symbols.get(w, str(w)) not in HYP_FILTER]
                    hyps[g0 + g][key] = ([symbols.get(rec["words"][i], str(rec["words"][i])) for i in keep],
                                         None if rec["conf"] is None else [float(rec["conf"][i]) for i in keep])
        if args.oracle:
            for (key, _), rec in zip(batch, wl.oracle([[word_id(w) for w in refs[k]] for k, _ in batch], skip_words=skip)):
                oracle[key] = rec
            for P in wl.packed:
                d = score.lattice_depth(P)
                if d is not None:
                    depth[0] += d[0]
                    depth[1] += d[1]
        del batch[:]

    for key, lat in kaldi_io.read_compact_lattice_ark(args.lat_file):
        if key not in refs:
            print("no reference for %s: skipped" % key)
            continue
        seen.add(key)
        order.append(key)
        batch.append((key, lat))
        if len(batch) >= args.batch_size:
            flush()
    flush()
    missing = [k for k in refs if k not in seen]
    for k in missing:
        print("no lattice for %s: its %d reference words count as errors" % (k, len(refs[k])))
    keys = [k for k in refs if k in seen]
    ref_words = sum(len(r) for r in refs.values())
    best = None
    for g, st in enumerate(settings):
        lmwt, wip = st[3]
        hw = [hyps[g][k][0] for k in keys]
        nz = [i for i, k in enumerate(keys) if hw[i]]           # an empty hypothesis costs len(ref), as utt_wer.py counts
        errs = {k: len(refs[k]) for k in keys}
        if nz:
            d = score.edit_distance([[word_id(w) for w in hw[i]] for i in nz], [[word_id(w) for w in refs[keys[i]]] for i in nz])
            for i, e in zip(nz, d):
                errs[keys[i]] = int(e)
        total = sum(errs.values()) + sum(len(refs[k]) for k in missing)
        with open(os.path.join(args.out_dir, "hyp_%d.%s.txt" % (lmwt, wip)), "w") as f:
            for k in keys:
                f.write(" ".join([k] + hyps[g][k][0]) + "\n")
        with open(os.path.join(args.out_dir, "result_%d_%s" % (lmwt, wip)), "w") as f:
            for k in keys:
                f.write("reco: %s %s\n" % (k, " ".join(hyps[g][k][0])))
                f.write("ref: %s %s\n" % (k, " ".join(refs[k])))
                f.write("%s err: %d ref_len: %d\n" % (k, errs[k], len(refs[k])))
                if args.decode_mbr:
                    f.write("conf: %s %s\n" % (k, " ".join("%.4f" % c for c in hyps[g][k][1])))
        if args.ctm:
            with open(os.path.join(args.out_dir, "ctm_%d_%s" % (lmwt, wip)), "w") as f:
                for k in order:
                    f.write("".join(line + "\n" for line in ctm[g][k]))
        if args.phone_ctm:
            with open(os.path.join(args.out_dir, "phone_ctm_%d_%s" % (lmwt, wip)), "w") as f:
                for k in order:
                    f.write("".join(line + "\n" for line in phone_ctm[g][k]))
        if best is None or total < best[0]:
            best = (total, lmwt, wip)
    if boundary is not None:
        print("aligned: %d of %d pairs, fallback: %d" % tuple(aligned))
    if args.oracle:
        tot = dict(errors=sum(len(refs[k]) for k in missing), ins=0, dele=sum(len(refs[k]) for k in missing), sub=0)
        with open(os.path.join(args.out_dir, "oracle.txt"), "w") as fh, open(os.path.join(args.out_dir, "result_oracle"), "w") as fr:
            for k in keys:
                rec = oracle[k]
                if rec["status"] != 0:       # a reference beyond the kernel's capacity: all its words count, as for a missing lattice
                    rec = dict(errors=len(refs[k]), ins=0, dele=len(refs[k]), sub=0, words=[])
                words = [symbols.get(w, str(w)) for w in rec["words"]]
                fh.write(" ".join([k] + words) + "\n")
                fr.write("reco: %s %s\n" % (k, " ".join(words)))
                fr.write("ref: %s %s\n" % (k, " ".join(refs[k])))
                fr.write("%s err: %d ref_len: %d\n" % (k, rec["errors"], len(refs[k])))
                fr.write("%s ins: %d del: %d sub: %d\n" % (k, rec["ins"], rec["dele"], rec["sub"]))
                for f in tot:
                    tot[f] += rec[f]
        print("oracle: errors=%d ref_words=%d WER=%.2f%% ins=%d del=%d sub=%d%s"
              % (tot["errors"], ref_words, 100.0 * tot["errors"] / max(1, ref_words), tot["ins"], tot["dele"], tot["sub"],
                 " depth=%.2f" % (depth[0] / depth[1]) if depth[1] > 0 else ""))
    print("best: LMWT=%d wip=%s errors=%d ref_words=%d WER=%.2f%%" % (best[1], best[2], best[0], ref_words,
                                                                      100.0 * best[0] / max(1, ref_words)))


if __name__ == "__main__":
    main()
