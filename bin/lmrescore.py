#!/usr/bin/env python
"""Rescores a compact-lattice archive with an n-gram LM -- the step between latgen.py and score*.sh of the reference's
OpenCSS recipe (local/lmrescore_const_arpa.sh: lattice-lmrescore --lm-scale=-1 ... G.fst | lattice-lmrescore-const-arpa
--lm-scale=1 ... G.carpa), running on libpk2hip.so: every lattice of a batch is composed with the LM by one workgroup of one
launch (pykaldi2_amd.score.rescore_lm).

  python bin/lmrescore.py -lat_file exp/se/lat.ark -new_lm data/lang/lm_big.arpa [-old_lm data/lang/lm_small.arpa] \
      -words_txt exp/tri/graph/words.txt [-lm_scale 1.0 -unk "<unk>"] -out_file exp/se/lat_rescored.ark

-old_lm (the LM of the decoding graph, ARPA text) is taken out with -lm_scale before -new_lm is put in with +lm_scale.
Lattice words that an LM has no unigram for are scored as -unk; without -unk such a word is an error.  Keys, acoustic costs
and the transition-id strings are kept; bin/score.py runs on the output unchanged.  No determinisation follows (Kaldi's
script determinises again): a determinised input stays deterministic on words, its states are split by LM history."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import kaldi_io, ngram, score  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("-lat_file", required=True, help="binary compact-lattice archive (bin/latgen.py -out_file)")
    parser.add_argument("-new_lm", required=True, help="ARPA file of the LM to put in")
    parser.add_argument("-old_lm", help="ARPA file of the LM to take out first (the decoding graph's)")
    parser.add_argument("-words_txt", required=True, help="the graph directory's words.txt")
    parser.add_argument("-lm_scale", default=1.0, type=float)
    parser.add_argument("-unk", help="the word that stands for lattice words an LM does not hold")
    parser.add_argument("-repair", action="store_true", help="skip n-grams whose context is not in the ARPA file")
    parser.add_argument("-out_file", required=True)
    parser.add_argument("-batch_size", default=32, type=int, help="lattices per device batch")
    parser.add_argument("-expand", default=8.0, type=float, help="room per lattice, in multiples of its size")
    parser.add_argument("-max_expand", default=64.0, type=float)
    args = parser.parse_args()

    load = lambda path: ngram.NgramLM.from_arpa(path, words_txt=args.words_txt, unk=args.unk, repair=args.repair)
    lms = []
    for path, scale in ((args.old_lm, -args.lm_scale), (args.new_lm, args.lm_scale)):
        if path:
            lm = load(path)
            print("%s: order %d, %d n-grams, %d skipped, scale %g" % (path, lm.order, lm.num_nodes - 1, lm.skipped, scale))
            lms.append((lm, scale))
    done, batch = [0, 0, 0], []

    def flush(writer):
        if not batch:
            return
        out = score.rescore_lm([lat for _, lat in batch], lms, "cuda", args.expand, args.max_expand, names=[k for k, _ in batch])
        for (key, lat), res in zip(batch, out):
            writer[key] = score.fold_finals(res)
            done[0] += 1
            done[1] += len(lat["arcs"])
            done[2] += int(res["src"].shape[0])
        del batch[:]

    with kaldi_io.CompactLatticeWriter("ark:" + args.out_file) as writer:
        for key, lat in kaldi_io.read_compact_lattice_ark(args.lat_file):
            batch.append((key, lat))
            if len(batch) >= args.batch_size:
                flush(writer)
        flush(writer)
    print("rescored %d lattices: %d arcs in, %d arcs out -> %s" % (done[0], done[1], done[2], args.out_file))


if __name__ == "__main__":
    main()
