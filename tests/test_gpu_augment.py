"""data.sequence_batches with data_config speed_perturb / volume_perturb (pykaldi2_amd.augment): nothing changes unless a key
asks for it, the perturbed minibatch is the restatement of Kaldi's resampler applied to the unperturbed draw, and the dynamic
simulation's own random draws stay what they are."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402

from pykaldi2_amd import augment, data  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _first_batch(source, batch_size=4):
    return next(data.sequence_batches(source, batch_size, 1.0, DEV))


def test_nothing_changes_without_a_perturbation():
    plain = data.SyntheticSource(120)                                # a source built with no augmentation at all
    off = data.make_source(dict(synthetic=True, data_config=dict(simulation_prob=0)), 120)
    noop = data.make_source(dict(synthetic=True, data_config=dict(speed_perturb=[1.0], volume_perturb=[1.0, 1.0])), 120)
    assert off.augment is None and noop.augment is not None
    a, b, c = _first_batch(plain), _first_batch(off), _first_batch(noop)
    assert a["lens"] == b["lens"] == c["lens"] and a["seconds"] == b["seconds"] == c["seconds"]
    assert torch.equal(a["wav"], b["wav"]) and torch.equal(a["wav"], c["wav"])
    assert "speed" not in a and "speed" not in b and c["speed"] == [1.0] * 4
    for ya, yb, yc in zip(a["y"], b["y"], c["y"]):
        assert np.array_equal(ya, yb) and np.array_equal(ya, yc)     # factor 1 keeps the labels


def test_speed_and_volume_perturbed_batch_matches_the_restatement():
    cfg = dict(synthetic=True, data_config=dict(speed_perturb=[0.9, 1.1], volume_perturb=[0.125, 2.0]))
    src = data.make_source(cfg, 120)
    batch = _first_batch(src)
    clean = _first_batch(data.SyntheticSource(120))
    factors, gains = src.augment.draw(src.augment.generator(0, 0), 4)
    assert batch["speed"] == factors and set(factors) <= {0.9, 1.1}
    assert batch["seconds"] == sum(batch["lens"]) / 16000.0 and batch["wav"].shape == (sum(batch["lens"]),)
    got, x_all = batch["wav"].cpu().numpy(), clean["wav"].cpu().numpy()
    a = b = 0
    for n in range(4):
        n_in, fi = clean["lens"][n], int(round(16000 * factors[n]))
        assert fi in (14400, 17600)
        assert batch["lens"][n] == -(-n_in * 16000 // fi)
        assert batch["y"][n] is None and clean["y"][n] is not None
        plan = augment.ResamplePlan(fi, 16000)
        first, taps, w = plan.export()
        want, B = RR.apply(x_all[a:a + n_in], plan.iu, plan.ou, first, taps, w, batch["lens"][n], gains[n])
        y = got[b:b + batch["lens"][n]]
        bound = (taps[np.arange(len(y)) % plan.ou] + 2) * 2.0 ** -24 * abs(gains[n]) * B
        err = np.abs(y - want)
        print("utterance %d: factor %.1f gain %.4f max err %.3e" % (n, factors[n], gains[n], err.max()))
        assert (err <= bound).all()
        a, b = a + n_in, b + batch["lens"][n]
    # the next epoch draws differently, the same epoch again draws the same
    assert src.augment.draw(src.augment.generator(0, 1), 64) != src.augment.draw(src.augment.generator(0, 0), 64)


def _simulated_batch(cfg, record):
    src = data.make_source(cfg, 120)
    pool = src.simulation
    sim, on_device = pool.sim, pool._on_device

    def spy_sim(*a, **k):
        y, sent = sim(*a, **k)
        record.append(("snr", [float(v) for v in sent.get("dir_snr", [])]))
        return y, sent

    def spy_pick(kind, idx, device):
        record.append((kind, idx))
        return on_device(kind, idx, device)
    pool.sim, pool._on_device = spy_sim, spy_pick
    np.random.seed(0)
    return src, _first_batch(src, 3)


def test_simulation_draws_are_untouched_and_the_gain_follows_it():
    dc = dict(simulation_prob=1.0, use_dir_noise=True, use_reverb=True, gain_norm=True)
    plain_draws, aug_draws = [], []
    _, plain = _simulated_batch(dict(synthetic=True, data_config=dict(dc)), plain_draws)
    src, pert = _simulated_batch(dict(synthetic=True, data_config=dict(dc, speed_perturb=[0.9, 1.1], volume_perturb=[0.25, 2.0])),
                                 aug_draws)
    assert len(plain_draws) == 3 * 4 and plain_draws == aug_draws          # noise pick, two RIR picks, SNR per utterance
    factors, gains = src.augment.draw(src.augment.generator(0, 0), 3)
    off = 0
    for n in range(3):
        fi = int(round(16000 * factors[n]))
        assert pert["lens"][n] == -(-plain["lens"][n] * 16000 // fi) and pert["y"][n] is None
        w = pert["wav"][off:off + pert["lens"][n]]
        assert torch.isfinite(w).all()
        # speed, then the simulation (peak-normalised to 0.5), then the volume gain
        assert abs(float(w.abs().max()) - 0.5 * gains[n]) < 1e-5 * max(1.0, gains[n])
        off += pert["lens"][n]
    assert off == pert["wav"].numel()
