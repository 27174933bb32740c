"""bin/train_chain.py -e2e (alignment-free LF-MMI) runs end to end on synthetic data in a fresh process: finite per-frame
losses, the skipped-utterance count in the progress line, the reference's checkpoint format."""
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


def test_train_chain_e2e_cli_synthetic(tmp_path):
    cfg = dict(data_config=dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=True,
                                load_label=True, use_cmn=True, simulation_prob=0),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    (tmp_path / "mmi.yaml").write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_chain.py"), "-config", str(tmp_path / "mmi.yaml"),
                          "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-3", "-batch_size", "4", "-sweep_size", "0.05",
                          "-print_freq", "1", "-xent_regularize", "0.1", "-e2e", "-synthetic", "-den_states", "400",
                          "-den_arcs", "6000", "-graph_words", "50"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("Epoch: [0]")]
    assert len(lines) >= 2, out.stdout[-2000:]
    for line in lines:
        m = re.search(r"Loss (\S+) \((\S+)\).*grad_norm (\S+) .*no_path (\d+) \((\d+)\)", line)
        assert m, line
        assert all(math.isfinite(float(v)) for v in m.groups()[:3]), line
        assert float(m.group(1)) != 0.0, line              # an objective was computed: not every utterance was skipped
    ck = torch.load(tmp_path / "exp" / "chain.model.0.tar", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch"} and "lstm.weight_hh_l1_reverse" in ck["model"]
