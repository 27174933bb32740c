"""Generates tests/golden/simulation_mask.npz by running the REFERENCE's own code (its `simulation` package:
SpectrumAnalyzer, MaskEstimator and istft of simulation/freq_analysis.py and simulation/mask.py; the checkout is the first
argument, /root/reference as in tools/gen_golden_simmc.py by default) on the seeded inputs of tests/mask_ref.py.  Run in the build
container only; the reference never travels, the fixture does.  The file holds outputs only (the inputs and the dither
are regenerated from their seeds), in the device's frame-major layout (N, F); masks as uint8.

    python tools/gen_golden_mask.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
np.int = int      # the reference uses the removed alias
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
from simulation.freq_analysis import SpectrumAnalyzer, istft          # noqa: E402
from simulation.mask import MaskEstimator                              # noqa: E402

import mask_ref as R                                              # noqa: E402

out = {}

# ---- MaskEstimator on the five cases, the analyzer's dither from np.random.seed (clean first, then distorted) ----
for name, case in R.MASK_CASES.items():
    clean, distorted = R.inputs(*case)
    np.random.seed(R.DITHER_SEED)
    m = MaskEstimator(SpectrumAnalyzer()).get_mask_from_parallel_data(clean, distorted)
    assert set(np.unique(m)) <= {0.0, 1.0}
    out[name + "_mask"] = m.T.astype(np.uint8)

# ---- analyze without dither and istft of that spectrum: the default configuration on the shortest case, the small ones ----
cases = {"m4": (R.DEFAULT, R.inputs(*R.MASK_CASES["m4"])[0])}
for name in ("hann64", "bartlett32"):
    cfg, n, seed = R.STFT_CASES[name]
    cases[name] = (cfg, R.inputs(seed, n, 5)[0])
for name, (cfg, x) in cases.items():
    an = SpectrumAnalyzer(dict(cfg, do_dither=False))
    spec = an.analyze(x)                                                # (F, N) complex64
    out[name + "_spec"] = spec.T.copy()
    out[name + "_istft"] = istft(spec.T, hop_length=cfg["frame_shift"], win_length=cfg["frame_len"], window=cfg["window"],
                                 center=False, dtype=np.float64)
# ... and one spectrum with the seeded dither
np.random.seed(R.DITHER_SEED)
out["m4_spec_dither"] = SpectrumAnalyzer().analyze(cases["m4"][1]).T.copy()

path = os.path.join(ROOT, "tests", "golden", "simulation_mask.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
