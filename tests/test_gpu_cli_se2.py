"""bin/train_se2.py (sequence training on alignments made on the fly) end to end: on the synthetic generators with MMI and
sMBR, and on recipe files on disk (binary final.mdl with <LogProbs>, tree, L.fst, disambig.int, word-id labels)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from pykaldi2_amd import synth

from recipe import lattice_recipe, model_yaml, write_fst_vector, write_labels
from test_align_graph import write_trans_model_binary

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODER = dict(beam=9.0, lattice_beam=4.0, max_active=400, acoustic_scale=0.3, align_beam=10)


def _run(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_se2.py")] + args, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch: [0]" in out.stdout and "grad_norm" in out.stdout
    losses = [float(v) for v in re.findall(r"Loss\s+(\S+)\s", out.stdout)]
    assert losses and all(np.isfinite(losses)), out.stdout[-2000:]
    return out


@pytest.mark.parametrize("criterion", ["mmi", "smbr"])
def test_train_se2_cli_synthetic(tmp_path, criterion):
    cfg = model_yaml(tmp_path / "se.yaml", 120, decoder=DECODER)
    _run(["-config", cfg, "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-4", "-momentum", "0.9", "-criterion", criterion,
          "-batch_size", "2", "-sweep_size", "0.02", "-print_freq", "1", "-synthetic", "-graph_words", "60"])
    ck = torch.load(tmp_path / "exp" / "model.se.0.tar", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch"} and "lstm.weight_hh_l1_reverse" in ck["model"]


def test_train_se2_cli_recipe_files(tmp_path):
    from pykaldi2_amd import lstm
    P, words = 90, 40
    r = lattice_recipe(str(tmp_path), P=P, words=words)
    tree, tm = synth.alignment_model(P)
    os.makedirs(tmp_path / "tri")
    write_trans_model_binary(str(tmp_path / "tri" / "final.mdl"), tm)
    tree.write(str(tmp_path / "tri" / "tree"))
    os.makedirs(tmp_path / "lang" / "phones")
    lex = synth.lexicon_arcs(words, P, seed=0)
    write_fst_vector(str(tmp_path / "lang" / "L.fst"), lex["num_states"], lex["start"], lex["src"], lex["dst"], lex["ilabel"],
                     lex["olabel"], lex["weight"], lex["final"])
    (tmp_path / "lang" / "phones" / "disambig.int").write_text("")
    rng = np.random.default_rng(0)
    texts = {utt: synth.word_transcript(rng, r["tids"][utt].shape[0], words) for utt in r["tids"]}
    write_labels(str(tmp_path / "data" / "words.txt"), texts)
    d = yaml.safe_load(open(tmp_path / "data" / "data.yaml"))
    d["clean_source"]["train"]["aux_label"] = str(tmp_path / "data" / "words.txt")
    (tmp_path / "data" / "data.yaml").write_text(yaml.safe_dump(d))
    torch.save({"model": lstm.LSTMAM(80, P, 64, 2, 0.0, True).state_dict()}, tmp_path / "seed.tar")
    cfg = model_yaml(tmp_path / "se.yaml", P, decoder=DECODER)
    _run(["-config", cfg, "-data", str(tmp_path / "data" / "data.yaml"), "-dataPath", "", "-exp_dir", str(tmp_path / "exp"),
          "-criterion", "mmi", "-seed_model", str(tmp_path / "seed.tar"), "-trans_model", str(tmp_path / "tri"),
          "-lang_dir", str(tmp_path / "lang"), "-prior_path", str(tmp_path / "final.occs"), "-den_dir",
          str(tmp_path / "graph"), "-lr", "1e-4", "-batch_size", "2", "-print_freq", "1"])
    assert os.path.isfile(tmp_path / "exp" / "model.se.0.tar")
