"""The command line with data_config beamform: train_ce.py trains on utterances that a simulated 7-microphone array heard
and the MVDR beamformer turned back into one channel; without online_rir it stops at start-up and names the key."""
import math
import os
import re
import subprocess
import sys

import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(tmp_path, **dc):
    data = dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=False, load_label=True, use_cmn=True,
                use_reverb=True, use_dir_noise=True, simulation_prob=1.0, gain_norm=True, beamform=True)
    data.update(dc)
    cfg = dict(data_config=data, model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    (tmp_path / "train.yaml").write_text(yaml.safe_dump(cfg))
    return str(tmp_path / "train.yaml")


def _train_ce(tmp_path, **dc):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_ce.py"), "-train_config", _config(tmp_path, **dc),
                           "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-3", "-batch_size", "16", "-sweep_size", "0.05",
                           "-print_freq", "1", "-synthetic"], capture_output=True, text=True, timeout=300)


def test_train_ce_trains_on_beamformed_audio_and_refuses_a_missing_online_rir(tmp_path):
    out = _train_ce(tmp_path, online_rir=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("Epoch: [0]")]
    assert len(lines) >= 1, out.stdout[-2000:]
    losses = []
    for line in lines:
        m = re.search(r"Loss\s+(\S+)\s+\((\S+)\).*grad_norm\s+(\S+)\s", line)
        assert m, line
        assert all(math.isfinite(float(v)) for v in m.groups()), line
        assert float(m.group(1)) != 0.0, line
        losses.append(float(m.group(2)))
    assert losses[-1] <= losses[0] * 1.05 and losses[-1] < 2 * math.log(120), losses      # the running mean does not climb
    assert (tmp_path / "exp" / "model.0.tar").exists()

    (tmp_path / "second").mkdir()
    out = _train_ce(tmp_path / "second")
    assert out.returncode != 0
    assert "online_rir" in out.stderr and "Traceback" not in out.stderr
    assert not (tmp_path / "second" / "exp" / "model.0.tar").exists()
