"""Generates tests/golden/simulation_mc.npz by running the REFERENCE's own simulation code
(its `simulation` package: Distorter with multi-channel RIRs and both noise placements, Mixer,
generate_isotropic_noise; the checkout is the first argument, /root/reference as in tools/gen_golden_sim.py by default) on the seeded inputs of tests/simmc_ref.py.  Run in the build container only; the reference
never travels, the fixture does.  The file holds outputs and scalars only (the inputs and the isotropic draws are
regenerated from their seeds), float64, in the device's channel-major layout (C, T).

    python tools/gen_golden_simmc.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
np.int = int      # the reference uses the removed alias
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
from simulation import _mixer                                         # noqa: E402
from simulation._distorter import Distorter                           # noqa: E402
from simulation._iso_noise_simulator import _get_hoth_mag, generate_isotropic_noise     # noqa: E402
from simulation._sampling import get_distribution_template, get_sample                  # noqa: E402

import simmc_ref as R                                            # noqa: E402

_mixer.get_sample = get_sample                                        # the two names _mixer.py forgot to import
_mixer.get_distribution_template = get_distribution_template
out = {}

# ---- Distorter.apply_rir with a (T, C) RIR and the early reverberation ----
for name in R.REVERB_CASES:
    wav, rir = R.inputs_reverb(name)
    rv, er = Distorter.apply_rir(wav.astype(np.float64), rir.astype(np.float64).T.copy(), get_early_reverb=True)
    out[name + "_out"], out[name + "_early"] = rv.T.copy(), er.T.copy()

# ---- Mixer.mix_signals ----
c = R.MIXER_CASE
sig, sig2 = R.inputs_mixer()
np.random.seed(c["draw_seed"])
mixed, _, starts, scale, pos2 = _mixer.Mixer(_mixer.MixerConfig().config).mix_signals(
    [x.astype(np.float64).T.copy() for x in sig], np.asarray(c["spr"]), signal2=[x.astype(np.float64).T.copy() for x in sig2])
out["mix_out"], out["mix_out2"] = mixed.T.copy(), sum(pos2).T.copy()      # (the second: the sum of positioned_source2)
out["mix_starts"], out["mix_scale"] = np.asarray(starts, np.int64), np.asarray(scale, np.float64).reshape(-1)

# ---- Distorter.add_noise, both placements ----
for name, c in R.NOISE_CASES.items():
    s, nz = R.inputs_noise(name)
    np.random.seed(c["draw_seed"])
    d, _ = Distorter.add_noise(s.astype(np.float64).T.copy(), nz.astype(np.float64).T.copy(), c["snr"], c["scheme"])
    np.random.seed(c["draw_seed"])
    out[name + "_start"] = np.int64(R.draw_noise_start(c["n"], c["m"], c["scheme"]))
    out[name + "_out"] = d.T.copy()

# ---- generate_isotropic_noise: the seed and the output, never the draws ----
for name, c in R.ISO_CASES.items():
    np.random.seed(c["seed"])
    out[name + "_out"] = generate_isotropic_noise(R.ISO_MICS, c["N"], c["fs"], type=c["type"], spectrum=c["spectrum"])
for fs, fft_size in ((16000, 4096), (16000, 2048), (8000, 2048)):
    out["hoth_%d_%d" % (fs, fft_size)] = _get_hoth_mag(fs, fft_size)

path = os.path.join(ROOT, "tests", "golden", "simulation_mc.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
