"""bin/latgen.py -> bin/lmrescore.py -> bin/score.py on synthetic data: the recipes' chain with LM rescoring in it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmrescore_ref as R  # noqa: E402
from pykaldi2_amd import kaldi_io  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 60


def _run(tool, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", tool)] + [str(a) for a in args], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_latgen_lmrescore_score(tmp_path):
    cfg = dict(data_config=dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=True, load_label=True,
                                use_cmn=True, simulation_prob=0),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120),
               decoder_config=dict(beam=11, lattice_beam=5, max_active=2000, acoustic_scale=0.1))
    (tmp_path / "se.yaml").write_text(yaml.safe_dump(cfg))
    _run("latgen.py", "-config", tmp_path / "se.yaml", "-out_file", tmp_path / "lat.ark", "-synthetic", 2, "-synthetic_words", WORDS,
         "-batch_size", 2)
    names = {w: "w%d" % w for w in range(1, WORDS + 1)}
    (tmp_path / "words.txt").write_text("<eps> 0\n" + "".join("%s %d\n" % (names[w], w) for w in range(1, WORDS + 1)))
    names[WORDS + 1], names[WORDS + 2] = "<s>", "</s>"
    # the old LM: the unigram of synth.decoding_graph_arcs (word w enters the loop at the Zipf cost ln w); the new one: a
    # small seeded bigram
    old = {(w,): (float(-np.log10(w)), None) for w in range(1, WORDS + 1)}
    old[(WORDS + 1,)], old[(WORDS + 2,)] = (-99.0, None), (0.0, None)
    R.write_arpa(str(tmp_path / "old.arpa"), old, 1, names)
    new, _, _ = R.random_lm(WORDS, 2, 9, density=0.05)
    R.write_arpa(str(tmp_path / "new.arpa"), new, 2, names)
    out = _run("lmrescore.py", "-lat_file", tmp_path / "lat.ark", "-old_lm", tmp_path / "old.arpa", "-new_lm", tmp_path / "new.arpa",
               "-words_txt", tmp_path / "words.txt", "-out_file", tmp_path / "res.ark")
    assert "rescored 2 lattices" in out
    before = list(kaldi_io.read_compact_lattice_ark(str(tmp_path / "lat.ark")))
    after = list(kaldi_io.read_compact_lattice_ark(str(tmp_path / "res.ark")))
    assert [k for k, _ in after] == [k for k, _ in before] == ["synth-1", "synth-2"]
    for (_, b), (_, a) in zip(before, after):
        # every arc of the output is a copy of an input arc between split states: same word, same acoustic cost, same
        # transition-id string; same for the final weights.
        sig = lambda lat: (set((x[3], x[4][1], tuple(x[4][2])) for x in lat["arcs"]),
                           set((f[1], tuple(f[2])) for f in lat["finals"] if np.isfinite(f[0])))
        (arcs_a, fin_a), (arcs_b, fin_b) = sig(a), sig(b)
        assert arcs_a and fin_a and arcs_a <= arcs_b and fin_a <= fin_b
        assert len(set((x[0], x[3]) for x in a["arcs"])) == len(a["arcs"])          # still deterministic on words
    (tmp_path / "text").write_text("synth-1 w1 w2 w3\nsynth-2 w4 w5\n")
    out = _run("score.py", "-lat_file", tmp_path / "res.ark", "-words_txt", tmp_path / "words.txt", "-ref_text", tmp_path / "text",
               "-out_dir", tmp_path / "scoring", "-min_lmwt", 9, "-max_lmwt", 10, "-word_ins_penalty", "0.0")
    assert out.strip().splitlines()[-1].startswith("best: LMWT=")
