"""bin/train_chain.py with data_config speed_perturb / volume_perturb: -e2e (alignment-free, frame counts from the perturbed
waveform) trains; without -e2e the labels are per frame of the unperturbed audio and the command line refuses at start-up."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(tmp_path):
    cfg = dict(data_config=dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=True,
                                load_label=True, use_cmn=True, simulation_prob=0, speed_perturb=[0.9, 1.0, 1.1],
                                volume_perturb=[0.125, 2.0]),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    (tmp_path / "mmi.yaml").write_text(yaml.safe_dump(cfg))
    return str(tmp_path / "mmi.yaml")


def _train_chain(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_chain.py"), "-config", _config(tmp_path),
                           "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-3", "-batch_size", "4", "-sweep_size", "0.05",
                           "-print_freq", "1", "-xent_regularize", "0.1", "-synthetic", "-den_states", "400",
                           "-den_arcs", "6000", "-graph_words", "50"] + list(extra),
                          capture_output=True, text=True, timeout=300)


def test_train_chain_e2e_trains_on_perturbed_audio(tmp_path):
    out = _train_chain(tmp_path, "-e2e")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("Epoch: [0]")]
    assert len(lines) >= 2, out.stdout[-2000:]
    for line in lines:
        m = re.search(r"Loss (\S+) \((\S+)\).*grad_norm (\S+) ", line)
        assert m, line
        assert all(math.isfinite(float(v)) for v in m.groups()), line
        assert float(m.group(1)) != 0.0, line
    ck = torch.load(tmp_path / "exp" / "chain.model.0.tar", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch"}


def test_train_chain_with_frame_labels_refuses_speed_perturb(tmp_path):
    out = _train_chain(tmp_path)
    assert out.returncode != 0
    assert "speed_perturb" in out.stderr and "Traceback" not in out.stderr
    assert not (tmp_path / "exp" / "chain.model.0.tar").exists()
