"""bin/train_se2.py -criterion mwe on the synthetic generators: word-level MWE against the transcripts, and phone-level MWE
against the on-the-fly alignments (`phone_level: true` in the YAML's mwe_config block)."""
import pytest
import yaml

from recipe import model_yaml
from test_gpu_cli_se2 import DECODER, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("phone_level", [False, True])
def test_train_se2_cli_mwe(tmp_path, phone_level):
    cfg = model_yaml(tmp_path / "se.yaml", 120, decoder=DECODER)
    with open(cfg) as f:
        c = yaml.safe_load(f)
    c["mwe_config"] = dict(num_paths=8, phone_level=phone_level)
    with open(cfg, "w") as f:
        yaml.safe_dump(c, f)
    _run(["-config", cfg, "-exp_dir", str(tmp_path / "exp"), "-lr", "1e-4", "-momentum", "0.9", "-criterion", "mwe",
          "-batch_size", "2", "-sweep_size", "0.02", "-print_freq", "1", "-synthetic", "-graph_words", "60"])
    assert (tmp_path / "exp" / "model.se.0.tar").exists()
