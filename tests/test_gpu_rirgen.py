"""Image-method RIRs on the device (csrc/rirgen.hip) against the reference's numpy `xp_rirgen`
(tests/golden/rirgen.npz), their reproducibility, and the online-RIR simulation of data.SimulationPool."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from pykaldi2_amd import data, rirgen, simulation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(golden):
    return golden("rirgen")


def _case(G, name):
    kw = dict(t60=None)
    for k in ("t60", "htw", "nsamples", "beta"):
        if name + "_" + k in G.files:
            kw[k] = G[name + "_" + k]
    kw["hpfilt"], kw["habets_compat"] = bool(G[name + "_hpfilt"]), bool(G[name + "_habets"])
    return dict(room=G[name + "_room"].reshape(3, 1), source_loc=G[name + "_src"], mic_loc=G[name + "_mic"], **kw)


def _names(G):
    return [str(n) for n in G["case_names"]]


def test_fixture_cases_match_the_reference(G):
    """atol = rtol = 1e-5: the reference's own bar between its numpy and cupy results."""
    for name in _names(G):
        got = rirgen.xp_rirgen(**_case(G, name))
        want = G[name + "_out"]
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape, name
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=1e-5, rtol=1e-5, err_msg=name)
    assert not G["htw_zero_out"].any()


def test_two_calls_are_bit_identical(G):
    for name in ("small_rich", "t60_multi", "habets"):
        a = rirgen.xp_rirgen(**_case(G, name)).cpu().numpy()
        b = rirgen.xp_rirgen(**_case(G, name)).cpu().numpy()
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name


def test_mixed_batch_equals_items_one_by_one(G):
    items = [_case(G, n) for n in _names(G)]
    batch = rirgen.rirgen_batch(items)
    for it, got, dl in zip(items, batch.rirs, batch.delays):
        alone = rirgen.rirgen_batch([it])
        assert np.array_equal(got.cpu().numpy().view(np.int32), alone.rirs[0].cpu().numpy().view(np.int32))
        assert torch.equal(dl, alone.delays[0])


def test_device_argmax_is_torch_argmax(G):
    b = rirgen.rirgen_batch([_case(G, n) for n in _names(G)])
    for r, dl in zip(b.rirs, b.delays):
        assert dl.dtype == torch.int32 and torch.equal(dl.long(), torch.argmax(r, dim=-1))


def test_sampled_batch_is_finite_and_starts_at_the_direct_path():
    np.random.seed(5)
    items = []
    for _ in range(64):
        room, t60, mic, src = rirgen.sample_online_room((0.1, 0.5), 2)
        items.append(dict(room=room, source_loc=src, mic_loc=mic, t60=t60))
    b = rirgen.rirgen_batch(items)
    for it, r, dl in zip(items, b.rirs, b.delays):
        assert torch.isfinite(r).all()
        direct = np.linalg.norm(it["source_loc"] - it["mic_loc"], axis=0) / (340 / 16000)      # samples, per source
        htw = rirgen.prepare(**it)["htw"]
        first = (r[:, 0].abs() > 0).int().argmax(dim=-1).cpu().numpy()       # nothing arrives before the direct path
        assert np.all(first >= np.floor(direct) - htw) and np.all(dl[:, 0].cpu().numpy() >= np.floor(direct) - htw)


def _pool(prob=1.0, gain_norm=True, online=True):
    cfg = dict(data_config=dict(simulation_prob=prob, use_dir_noise=True, use_reverb=True, gain_norm=gain_norm,
                                online_rir=online), synthetic=True)
    return data.SimulationPool.from_config(cfg, seed=0)


def test_online_pool_equals_simple_simulator_by_hand():
    """The pool's draws (simulate?, noise, room, T60, mic, sources, SNR, noise position) replayed by hand with
    xp_rirgen and SimpleSimulator (host argmax): the same waveform, bit for bit."""
    dev = torch.device("cuda")
    pool = _pool()
    wavs = [np.random.default_rng(k).standard_normal(16000 * (2 + k)).astype(np.float32) * 0.1 for k in range(3)]
    np.random.seed(77)
    got = [pool.maybe_simulate(w, dev).cpu().numpy() for w in wavs]
    np.random.seed(77)
    sim = simulation.SimpleSimulator(use_rir=True, use_noise=True)
    for w, g in zip(wavs, got):
        assert not np.random.random() > 1.0
        noise = torch.from_numpy(pool.noises[int(np.random.choice(len(pool.noises)))]).to(dev)
        room, t60, mic, src = rirgen.sample_online_room((0.1, 0.5), 2)
        r = rirgen.xp_rirgen(room, src, mic, t60=t60)
        y, _ = sim(torch.from_numpy(w).to(dev), [noise], r[0, 0].contiguous(), [r[1, 0].contiguous()], normalize_gain=True)
        assert np.array_equal(y.cpu().numpy().view(np.int32), g.view(np.int32))
        assert abs(float(np.abs(g).max()) - 0.5) < 1e-5


def test_online_minibatch_makes_no_host_synchronisation():
    """torch's sync debug mode raises on every synchronising call torch makes (.item(), a blocking copy, ...)."""
    src = data.make_source(dict(data_config=dict(simulation_prob=1.0, use_dir_noise=True, use_reverb=True, gain_norm=True,
                                                 online_rir=True), synthetic=True), 120)
    np.random.seed(3)
    it = data.sequence_batches(src, 4, 1.0, torch.device("cuda"))
    next(it)                                                     # first call: allocations, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = next(it)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(b["wav"]).all() and b["wav"].numel() == sum(b["lens"])


def test_train_ce_cli_with_online_rir(tmp_path):
    cfg = dict(data_config=dict(frame_len=400, frame_shift=160, seg_len=80, seg_shift=80, sequence_mode=False,
                                load_label=True, use_cmn=True, simulation_prob=1, use_reverb=True, use_dir_noise=True,
                                online_rir=True, t60_range=[0.1, 0.5]),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    p = tmp_path / "ce.yaml"
    p.write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_ce.py"), "-train_config", str(p), "-exp_dir",
                          str(tmp_path / "exp"), "-lr", "1e-3", "-batch_size", "8", "-sweep_size", "0.03", "-print_freq", "1",
                          "-synthetic"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch: [0]" in out.stdout
    losses = [float(v) for v in re.findall(r"Loss ([^ ()]+) \(", out.stdout)]
    assert losses and all(np.isfinite(losses))
