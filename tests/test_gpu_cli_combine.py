"""bin/score.py -combine (MBR system combination) on archives written with the project's own writer: its
hyp_* files are CombinedBatch.mbr's words on the lattices read back, its result_* files and the `best:` line agree with
score.wer, and the flags it cannot serve are refused at start-up."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as R  # noqa: E402
from pykaldi2_amd import kaldi_io, score  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = os.path.join(ROOT, "bin", "score.py")


def folded(lat):
    """A generator lattice in the archive writer's form: packed to a single end state, the end arcs folded into finals."""
    P = score.pack_lattice(lat)
    final = np.full(P.S, np.inf, np.float32)
    final[P.S - 1] = 0.0
    raw = dict(num_states=P.S, start=0, src=P.src, dst=P.dst, word=P.word_ids[P.word], graph=P.graph, acoustic=P.acoustic,
               final=final)
    return score.fold_finals(raw)


def write_ark(path, table):
    with kaldi_io.CompactLatticeWriter("ark:" + str(path)) as w:
        for k, v in table.items():
            w[k] = v


def test_score_cli_combines_three_archives(tmp_path):
    keys = ["utt1", "utt2", "utt3"]
    systems = [{k: folded(R.random_lattice(8, 4, 5, seed=10 * s + i)) for i, k in enumerate(keys)} for s in range(3)]
    del systems[2]["utt2"]                            # the third system has no lattice for utt2
    paths = [tmp_path / ("lat%d.ark" % s) for s in range(3)]
    for p, t in zip(paths, systems):
        write_ark(p, t)
    sym = {0: "<eps>", 1: "A", 2: "B", 3: "C", 4: "<UNK>", 5: "E"}
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (s, i) for i, s in sym.items()))
    refs = {"utt1": ["A", "B", "C", "A", "E", "B", "C", "A"], "utt2": ["B", "B", "E", "C", "A", "A", "C"],
            "utt3": ["C", "A", "B", "E", "E", "B", "A", "C", "B"]}
    (tmp_path / "text").write_text("".join("%s %s\n" % (k, " ".join(v)) for k, v in refs.items()))
    out_dir = tmp_path / "out"
    run = subprocess.run([sys.executable, SCORE, "-lat_file", str(paths[0]), "-combine", "%s,%s" % (paths[1], paths[2]),
                          "-lat_weights", "0.5:0.3:0.2", "-words_txt", str(tmp_path / "words.txt"), "-ref_text",
                          str(tmp_path / "text"), "-out_dir", str(out_dir), "-min_lmwt", "9", "-max_lmwt", "10",
                          "-word_ins_penalty", "0.0,1.0"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "no lattice for utt2 in %s" % paths[2] in run.stdout
    settings = score.sweep(9, 10, (0.0, 1.0))
    assert sorted(os.listdir(out_dir)) == sorted(["hyp_%d.%s.txt" % st[3] for st in settings] + ["result_%d_%s" % st[3] for st in settings])
    read = [dict(kaldi_io.read_compact_lattice_ark(str(p))) for p in paths]
    recs = score.CombinedBatch([[t.get(k) for k in keys] for t in read], names=keys, weights=[0.5, 0.3, 0.2]).mbr(settings)
    ids = {s: i for i, s in sym.items()}
    totals = []
    for g, st in enumerate(settings):
        lmwt, wip = st[3]
        hyps = [[sym[w] for w in recs[u][g]["words"] if sym[w] != "<UNK>"] for u in range(3)]
        lines = (out_dir / ("hyp_%d.%s.txt" % (lmwt, wip))).read_text().splitlines()
        assert lines == [" ".join([k] + h) for k, h in zip(keys, hyps)]
        errs, nref = score.wer([[ids[w] for w in h] for h in hyps], [[ids[w] for w in refs[k]] for k in keys])
        res = (out_dir / ("result_%d_%s" % (lmwt, wip))).read_text().splitlines()
        assert len(res) == 4 * 3 and sum(int(l.split()[2]) for l in res if " err: " in l) == errs
        for u, k in enumerate(keys):
            each = score.wer([[ids[w] for w in hyps[u]]], [[ids[w] for w in refs[k]]])[0]
            assert "%s err: %d ref_len: %d" % (k, each, len(refs[k])) in res
            conf = [float(c) for w, c in zip(recs[u][g]["words"], recs[u][g]["conf"]) if sym[w] != "<UNK>"]
            assert "conf: %s %s" % (k, " ".join("%.4f" % c for c in conf)) in [l.rstrip() for l in res]
        totals.append((errs, lmwt, wip))
        assert nref == 24
    best = min(totals, key=lambda t: t[0])
    assert run.stdout.strip().splitlines()[-1] == "best: LMWT=%d wip=%s errors=%d ref_words=24 WER=%.2f%%" % (
        best[1], best[2], best[0], 100.0 * best[0] / 24)


def test_score_cli_refuses_ctm_and_oracle_with_combine(tmp_path):
    write_ark(tmp_path / "a.ark", {"utt1": folded(R.random_lattice(3, 2, 3, seed=0))})
    (tmp_path / "words.txt").write_text("<eps> 0\nA 1\n")
    (tmp_path / "text").write_text("utt1 A\n")
    base = [sys.executable, SCORE, "-lat_file", str(tmp_path / "a.ark"), "-combine", str(tmp_path / "a.ark"), "-words_txt",
            str(tmp_path / "words.txt"), "-ref_text", str(tmp_path / "text"), "-out_dir", str(tmp_path / "out")]
    for flag in ("-ctm", "-oracle"):
        run = subprocess.run(base + [flag], capture_output=True, text=True, timeout=300)
        assert run.returncode != 0 and flag in run.stderr and "-combine" in run.stderr
        assert not os.path.exists(tmp_path / "out")
