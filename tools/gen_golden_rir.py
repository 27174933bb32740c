"""Generates tests/golden/rirgen.npz by running the REFERENCE's own image-method RIR generator (simulation/_rirgen.py
`xp_rirgen`, numpy) and its room / array / source sampling functions (simulation/_sampling.py with the default
RoomConfig / ArrayPositionConfig / SoundSourceConfig) on fixed inputs and a fixed seed.  Needs a checkout of the
reference project; only the fixture is kept.

    python tools/gen_golden_rir.py REFERENCE_CHECKOUT
"""
import os
import sys

import numpy as np

np.int = int      # the reference uses the removed alias
sys.path.insert(0, sys.argv[1])
from simulation._rirgen import xp_rirgen, min_t60_of_room              # noqa: E402
from simulation._geometry import RoomConfig, ArrayPositionConfig, SoundSourceConfig  # noqa: E402
from simulation._sampling import (get_distribution_template, get_sample, sample_room, sample_array_position,  # noqa: E402
                                  sample_source_position_by_random_coordinate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rng = np.random.default_rng(20261016)
out = {}

# name: room, sources (3, nsrc), mics (3, nmic), keyword arguments of xp_rirgen
room_a = np.array([4.0, 7.0, 3.0]).reshape(3, 1)
CASES = {
    "t60_multi": (room_a, rng.uniform(0.1, 0.9, (3, 2)) * room_a, rng.uniform(0.1, 0.9, (3, 3)) * room_a, dict(t60=0.3)),
    "beta_walls": (room_a, rng.uniform(0.1, 0.9, (3, 2)) * room_a, rng.uniform(0.1, 0.9, (3, 2)) * room_a,
                   dict(beta=rng.uniform(0.1, 0.9, size=6), t60=None)),
    "small_rich": (np.array([3.0, 3.0, 2.5]).reshape(3, 1), np.array([[1.1], [0.8], [1.5]]), np.array([[2.2], [2.1], [1.2]]),
                   dict(t60=0.5)),
    "large_short": (np.array([18.5, 14.0, 4.6]).reshape(3, 1), np.array([[3.0], [9.5], [1.7]]), np.array([[10.2], [6.1], [1.1]]),
                    dict(t60=0.31)),
    "explicit_htw_ns": (room_a, np.array([[1.0], [2.0], [1.5]]), np.array([[3.1], [5.2], [1.2]]),
                        dict(t60=0.4, htw=8, nsamples=3000)),
    "no_hpfilt": (room_a, np.array([[2.5], [1.2], [2.0]]), np.array([[0.7], [4.4], [1.4]]), dict(t60=0.25, hpfilt=False)),
    "habets": (np.array([5.0, 4.0, 3.0]).reshape(3, 1), np.array([[1.0], [1.5], [1.7]]), np.array([[3.5], [2.2], [1.3]]),
               dict(t60=0.3, habets_compat=True)),
    "near_wall": (np.array([6.0, 5.0, 3.0]).reshape(3, 1), np.array([[0.05], [2.5], [1.6]]), np.array([[3.0], [2.0], [1.5]]),
                  dict(t60=0.35)),
    "htw_zero": (np.array([0.2, 1.5, 1.2]).reshape(3, 1), np.array([[0.1], [0.4], [0.5]]), np.array([[0.12], [1.1], [0.7]]),
                 dict(t60=0.2)),
}
names = sorted(CASES)
out["case_names"] = np.array(names)
for name in names:
    room, src, mic, kw = CASES[name]
    r = xp_rirgen(room, src, mic, **kw)
    out[name + "_room"], out[name + "_src"], out[name + "_mic"] = room[:, 0], src, mic
    out[name + "_out"] = np.asarray(r, dtype=np.float32) if not kw.get("habets_compat") else np.asarray(r)
    for k in ("t60", "htw", "nsamples"):
        if kw.get(k) is not None:
            out[name + "_" + k] = np.asarray(kw[k])
    if kw.get("beta") is not None:
        out[name + "_beta"] = kw["beta"]
    out[name + "_hpfilt"] = np.int64(kw.get("hpfilt", True))
    out[name + "_habets"] = np.int64(kw.get("habets_compat", False))
    print(name, r.shape, r.dtype, float(np.abs(r).max()))

# ---- the online-RIR draws: room, T60 raised to the room's minimum, mic at the array centre, speech + noise source ----
SEED, N = 1234, 24
np.random.seed(SEED)
t60_cfg = get_distribution_template("T60", max=0.5, min=0.1, distribution="uniform")
rooms, t60s, mics, srcs = [], [], [], []
for _ in range(N):
    room = sample_room(RoomConfig().config)
    t60 = max(float(get_sample(t60_cfg)[0]), float(min_t60_of_room(room)))
    array = sample_array_position(ArrayPositionConfig(np.zeros((3, 1))).config, room)
    src = sample_source_position_by_random_coordinate(SoundSourceConfig().config, 2, room, array["array_ctr"][:, 0])
    rooms.append(room), t60s.append(t60), mics.append(array["mic_position"]), srcs.append(src)
out["sample_seed"] = np.int64(SEED)
out["sample_rooms"], out["sample_t60"] = np.array(rooms), np.array(t60s)
out["sample_mics"], out["sample_srcs"] = np.array(mics), np.array(srcs)

path = os.path.join(ROOT, "tests", "golden", "rirgen.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
