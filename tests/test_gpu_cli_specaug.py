"""The command lines with data_config spec_augment: the masks train everywhere; a time warp moves frames under frame-level
labels, so train_chain.py refuses it at start-up unless -e2e takes the supervision from the transcripts."""
import math
import os
import re
import subprocess
import sys

import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODER = dict(beam=9.0, lattice_beam=4.0, max_active=400, acoustic_scale=0.3, align_beam=10)


def _config(tmp_path, spec, sequence_mode=True, decoder=None):
    cfg = dict(data_config=dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=sequence_mode,
                                load_label=True, use_cmn=True, simulation_prob=0, spec_augment=spec),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    if decoder:
        cfg["decoder_config"] = decoder
    (tmp_path / "train.yaml").write_text(yaml.safe_dump(cfg))
    return str(tmp_path / "train.yaml")


def _run(prog, args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args, capture_output=True, text=True, timeout=300)


def _train_chain(tmp_path, spec, *extra):
    return _run("train_chain.py", ["-config", _config(tmp_path, spec), "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-3",
                                   "-batch_size", "4", "-sweep_size", "0.05", "-print_freq", "1", "-xent_regularize", "0.1",
                                   "-synthetic", "-den_states", "400", "-den_arcs", "6000", "-graph_words", "50"] + list(extra))


def _trained(out, least=2):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("Epoch: [0]")]
    assert len(lines) >= least, out.stdout[-2000:]
    for line in lines:
        m = re.search(r"Loss\s+(\S+)\s+\((\S+)\).*grad_norm\s+(\S+)\s", line)
        assert m, line
        assert all(math.isfinite(float(v)) for v in m.groups()), line
        assert float(m.group(1)) != 0.0, line


def test_train_chain_with_frame_labels_trains_on_masked_features(tmp_path):
    _trained(_train_chain(tmp_path, {"time_warp": 0}))
    assert (tmp_path / "exp" / "chain.model.0.tar").exists()


def test_train_chain_with_frame_labels_refuses_a_time_warp(tmp_path):
    out = _train_chain(tmp_path, {"time_warp": 5})
    assert out.returncode != 0
    assert "time_warp" in out.stderr and "Traceback" not in out.stderr
    assert not (tmp_path / "exp" / "chain.model.0.tar").exists()


def test_train_chain_e2e_trains_on_warped_features(tmp_path):
    _trained(_train_chain(tmp_path, {"time_warp": 5}, "-e2e"))
    assert (tmp_path / "exp" / "chain.model.0.tar").exists()


def test_train_ce_trains_on_masked_features(tmp_path):
    out = _run("train_ce.py", ["-train_config", _config(tmp_path, True, sequence_mode=False), "-exp_dir", str(tmp_path / "exp"),
                               "-lr", "1e-3", "-batch_size", "16", "-sweep_size", "0.05", "-print_freq", "1", "-synthetic"])
    _trained(out, least=1)
    assert (tmp_path / "exp" / "model.0.tar").exists()


def test_train_se2_teacher_student_trains_on_masked_features(tmp_path):
    out = _run("train_se2.py", ["-config", _config(tmp_path, True, decoder=DECODER), "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-4",
                                "-momentum", "0.9", "-criterion", "ts", "-batch_size", "2", "-sweep_size", "0.02", "-print_freq",
                                "1", "-synthetic", "-graph_words", "60"])
    _trained(out, least=1)
    assert (tmp_path / "exp" / "model.se.0.tar").exists()


def test_an_unknown_key_stops_the_command_line(tmp_path):
    out = _train_chain(tmp_path, {"time_wrap": 5})
    assert out.returncode != 0 and "time_wrap" in out.stderr
    assert not (tmp_path / "exp" / "chain.model.0.tar").exists()
