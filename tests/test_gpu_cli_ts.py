"""bin/train_se2.py -criterion ts (lattice teacher-student training) end to end on the synthetic generators: with the default
teacher (the student's configuration, another seed) and with a `teacher_config` of another hidden size."""
import pytest
import torch
import yaml

from recipe import model_yaml
from test_gpu_cli_se2 import DECODER, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("teacher", ["default", "wider"])
def test_train_se2_cli_teacher_student(tmp_path, teacher):
    cfg = model_yaml(tmp_path / "se.yaml", 120, decoder=DECODER)
    if teacher == "wider":
        with open(cfg) as f:
            c = yaml.safe_load(f)
        c["teacher_config"] = dict(hidden_size=128)     # the recurrence kernels serve 64, 128, 256, 512, 1024
        c["ts_config"] = dict(am_weight=0.3, lm_weight=1.0, old_acoustic_scale=0.0)
        with open(cfg, "w") as f:
            yaml.safe_dump(c, f)
    out = _run(["-config", cfg, "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-4", "-momentum", "0.9", "-criterion", "ts",
                "-batch_size", "2", "-sweep_size", "0.02", "-print_freq", "1", "-synthetic", "-graph_words", "60"])
    assert "Warning" not in out.stdout
    ck = torch.load(tmp_path / "exp" / "model.se.0.tar", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch"} and "lstm.weight_hh_l1_reverse" in ck["model"]
    assert ck["model"]["lstm.weight_hh_l0"].shape[1] == 64      # the student's size, whatever the teacher's
