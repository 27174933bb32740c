"""Multi-channel / multi-source simulation on the device against the reference's own outputs
(tests/golden/simulation_mc.npz) and the float64 restatement tests/simmc_ref.py: batched reverberation with early
reverberation, Mixer, both noise placements over C channels, the whole MultiSourceSimulator, and the isotropic noise
field (explicit draws against the reference, the in-kernel generator against its host restatement, the field's spatial
coherence against the quadrature over the 512 directions).  Device layout: channel-major (C, T)."""
import numpy as np
import pytest

import simmc_ref as R

pytestmark = pytest.mark.gpu

# float32 kernels against float64 references.  The rule: run the restatement once in float32 on the CPU
# against the float64 result and take 4 x its largest error relative to max|want| -- that covers the kernels' different
# summation order and the float32 sincos / log / sqrt.
ISO_TOL = 4 * 5.47e-7        # simmc_ref.iso_noise(float32) against the golden: 5.01e-7 .. 5.47e-7 over the five cases
GAUSS_TOL = 4 * 4.56e-7      # simmc_ref.gauss_host(float32) against float64 over 512 x 2049 pairs (max |z| = 5.2)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def G(golden):
    return golden("simulation_mc")


# ---------------------------------------------------------------------------------------------------------------------
# reverberation: 2 sources x 3 channels in one launch, n = 1500 / 1100, k = 1500 / 257, delays 7 / 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay", ["int", "device", "argmax"])
def test_gpu_batched_reverb_matches_reference(G, delay):
    import torch
    from pykaldi2_amd import simulation
    names = sorted(R.REVERB_CASES)
    wavs, rirs = zip(*[R.inputs_reverb(n) for n in names])
    d_wavs, d_rirs = [dev(w) for w in wavs], [dev(r) for r in rirs]
    if delay == "int":
        delays = [R.REVERB_CASES[n]["delay"] for n in names]
    elif delay == "device":       # a row of rirgen's `delays`: the argmax of every channel, the first one is used
        delays = [torch.from_numpy(np.argmax(r, axis=1).astype(np.int32)).cuda() for r in rirs]
    else:
        delays = [None, None]
    reverb, early = simulation._apply_rir_batch(d_wavs, d_rirs, delays, get_early_reverb=True)
    for i, n in enumerate(names):
        for got, want in ((reverb[i], G[n + "_out"]), (early[i], G[n + "_early"])):
            got = got.cpu().numpy()
            assert got.shape == want.shape
            err = np.abs(got - want).max()
            print(n, delay, "err %.3e bound %.3e" % (err, 2e-6 * np.abs(want).max() + 1e-7))
            assert err <= 2e-6 * np.abs(want).max() + 1e-7
        assert np.array_equal(d_wavs[i].cpu().numpy(), wavs[i]) and np.array_equal(d_rirs[i].cpu().numpy(), rirs[i])
        # the public entry gives the same rows, and without the early output too
        rv, er = simulation.Distorter.apply_rir(d_wavs[i], d_rirs[i], delays[i], get_early_reverb=True)
        assert torch.equal(rv, reverb[i]) and torch.equal(er, early[i])
        assert torch.equal(simulation.Distorter.apply_rir(d_wavs[i], d_rirs[i], delays[i]), reverb[i])
    # channel 0 is the single-channel kernel's result bit for bit (one tile function), and the early reverberation is the
    # running sum at the cut: the reverberation by the RIR cut to min(k, 640 + delay) = 647 taps
    c = R.REVERB_CASES["rev_a"]
    i = names.index("rev_a")
    assert torch.equal(simulation.Distorter.apply_rir(d_wavs[i], d_rirs[i][0].contiguous(), c["delay"]), reverb[i][0])
    cut = 640 + c["delay"]
    assert torch.equal(simulation.Distorter.apply_rir(d_wavs[i], d_rirs[i][:, :cut].contiguous(), c["delay"]), early[i])
    j = names.index("rev_b")
    assert torch.equal(early[j], reverb[j])          # k = 257 is shorter than the cut


# ---------------------------------------------------------------------------------------------------------------------
# Mixer: lengths 4000 / 2500 / 4000, spr = (1.5, -2.0), signal2 given
# ---------------------------------------------------------------------------------------------------------------------
def test_gpu_mixer_matches_reference(G):
    import torch
    from pykaldi2_amd import simulation
    c = R.MIXER_CASE
    sig, sig2 = R.inputs_mixer()
    d_sig, d_sig2 = [dev(x) for x in sig], [dev(x) for x in sig2]
    np.random.seed(c["draw_seed"])
    mixed, pos, starts, scale, pos2 = simulation.Mixer(simulation.MixerConfig()).mix_signals(d_sig, np.asarray(c["spr"]), signal2=d_sig2)
    assert starts == G["mix_starts"].tolist()
    assert scale.shape == (3, 1) and scale.dtype == torch.float64 and scale.is_cuda
    assert np.abs(scale.cpu().numpy().reshape(-1) / G["mix_scale"] - 1).max() < 1e-12
    want = G["mix_out"]
    err = np.abs(mixed.cpu().numpy() - want).max()
    print("mixer err %.3e bound %.3e" % (err, 5e-6 * np.abs(want).max()))
    assert err <= 5e-6 * np.abs(want).max()
    want2 = G["mix_out2"]
    assert np.abs(sum(p.cpu().numpy().astype(np.float64) for p in pos2) - want2).max() <= 5e-6 * np.abs(want2).max()
    _, _, ref_pos2 = R.mix(sig, c["spr"], starts, sig2)
    for i in range(3):
        assert np.abs(pos2[i].cpu().numpy() - ref_pos2[i]).max() <= 5e-6 * np.abs(ref_pos2[i]).max()
        p = np.zeros((c["C"], 4000), np.float32)
        p[:, starts[i]:starts[i] + c["lengths"][i]] = sig[i]
        assert np.array_equal(pos[i].cpu().numpy(), p)                       # positioned, unscaled
        assert np.array_equal(d_sig[i].cpu().numpy(), sig[i]) and np.array_equal(d_sig2[i].cpu().numpy(), sig2[i])
    # spr = None: n - 1 uniforms over the SPR range first, then the start of the one shorter source
    np.random.seed(77)
    got = simulation.Mixer(simulation.MixerConfig((-2.5, 2.5))).mix_signals(d_sig)
    rs = np.random.RandomState(77)
    spr = rs.uniform(low=-2.5, high=2.5, size=2)
    assert len(got) == 4 and got[2] == [0, int(rs.randint(0, high=1500, size=1)[0]), 0]
    want, _, _ = R.mix(sig, spr, got[2])
    assert np.abs(got[0].cpu().numpy() - want).max() <= 5e-6 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# noise placement: 'repeat_noise' (m = 1300 -> n = 4000, m = 9000 -> n = 3000, equal) and 'sample_noise' at C = 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.NOISE_CASES))
def test_gpu_add_noise_mc_matches_reference(G, name):
    from pykaldi2_amd import simulation
    c = R.NOISE_CASES[name]
    sig, nz = R.inputs_noise(name)
    d_sig, d_nz = dev(sig), dev(nz)
    np.random.seed(c["draw_seed"])             # the reference's own draw of the noise position
    got, start = simulation.Distorter.add_noise(d_sig, d_nz, c["snr"], noise_position_scheme=c["scheme"])
    assert start == int(G[name + "_start"])
    want = G[name + "_out"]
    err = np.abs(got.cpu().numpy() - want).max()
    print(name, "err %.3e bound %.3e" % (err, 2e-6 * np.abs(want).max()))
    assert got.shape == want.shape and err <= 2e-6 * np.abs(want).max()
    assert np.array_equal(d_sig.cpu().numpy(), sig) and np.array_equal(d_nz.cpu().numpy(), nz)       # inputs are left alone


# ---------------------------------------------------------------------------------------------------------------------
# the whole simulator against the restatement under the same seed
# ---------------------------------------------------------------------------------------------------------------------
def _utterance():
    wavs, rirs = zip(*[R.inputs_reverb(n) for n in sorted(R.REVERB_CASES)])
    rs = np.random.RandomState(401)
    noises = [R.make_wav(rs, 900, 0.2), R.make_wav(rs, 2000, 0.2)]          # shorter / longer than the 1500-sample mixture
    noise_rirs = [R.make_rir(rs, 300, 12, 3), R.make_rir(rs, 300, 5, 3)]
    iso = R.make_wav(rs, 700, 0.1, 3)                                       # repeated three times
    return list(wavs), list(rirs), noises, noise_rirs, iso


def _check_cfg(cfg, want):
    assert set(cfg) == set(want)
    for k in want:
        if k in ("scale", "gain_norm_scale"):          # device tensors; float32 signals behind them
            assert cfg[k].is_cuda and np.abs(cfg[k].cpu().numpy().reshape(-1) / np.asarray(want[k]).reshape(-1) - 1).max() < 1e-5
        elif isinstance(want[k], np.ndarray):
            assert np.array_equal(cfg[k], want[k]), k
        else:
            assert cfg[k] == want[k], k


@pytest.mark.parametrize("normalize_gain", [True, False])
def test_gpu_multi_source_simulator_matches_restatement(normalize_gain):
    from pykaldi2_amd import simulation
    wavs, rirs, noises, noise_rirs, iso = _utterance()
    sim = simulation.MultiSourceSimulator(array_geometry=np.zeros((3, 3)), use_rir=True, use_noise=True, snr_range=(0, 30),
                                          n_source_range=(2, 2), spr_range=(-2.5, 2.5))
    np.random.seed(61)
    mixed, early, mask, cfg = sim([dev(w) for w in wavs], [dev(x) for x in noises], [dev(r) for r in rirs],
                                  [dev(r) for r in noise_rirs], dev(iso), gen_mask=False, normalize_gain=normalize_gain,
                                  get_early_reverb=True)
    np.random.seed(61)
    want, want_early, want_cfg = R.simulate(wavs, noises, rirs, noise_rirs, iso, normalize_gain, True)
    assert mask is None and mixed.shape == (3, 1500) and len(early) == 2
    _check_cfg(cfg, want_cfg)
    err = np.abs(mixed.cpu().numpy() - want).max()
    print("simulator err %.3e bound %.3e" % (err, 5e-6 * np.abs(want).max()))
    assert err <= 5e-6 * np.abs(want).max()
    for g, w in zip(early, want_early):
        assert g.shape == (3, 1500) and np.abs(g.cpu().numpy() - w).max() <= 5e-6 * np.abs(w).max()
    if normalize_gain:
        assert abs(float(mixed.abs().max()) - 0.5) < 1e-6
    # without the early output
    np.random.seed(61)
    again, none, _, cfg2 = sim([dev(w) for w in wavs], [dev(x) for x in noises], [dev(r) for r in rirs],
                               [dev(r) for r in noise_rirs], dev(iso), normalize_gain=normalize_gain)
    # (equal up to the order in which the power sums' float64 partial sums are added)
    assert none is None and np.abs(again.cpu().numpy() - mixed.cpu().numpy()).max() <= 1e-6 * np.abs(want).max()


def test_gpu_simple_simulator_multichannel_matches_restatement():
    from pykaldi2_amd import simulation
    wavs, rirs, noises, noise_rirs, _ = _utterance()
    sim = simulation.SimpleSimulator(array_geometry=np.zeros((3, 3)), use_rir=True, use_noise=True)
    np.random.seed(62)
    mixed, cfg = sim(dev(wavs[0]), [dev(x) for x in noises], dev(rirs[0]), [dev(r) for r in noise_rirs])
    np.random.seed(62)
    want, _, want_cfg = R.simulate(wavs[:1], noises, rirs[:1], noise_rirs, None, True, False)
    _check_cfg(cfg, want_cfg)
    assert mixed.shape == (3, 1500) and np.abs(mixed.cpu().numpy() - want).max() <= 5e-6 * np.abs(want).max()
    assert abs(float(mixed.abs().max()) - 0.5) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# isotropic noise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.ISO_CASES))
def test_gpu_isotropic_noise_with_explicit_draws_matches_reference(G, name):
    from pykaldi2_amd import simulation
    c = R.ISO_CASES[name]
    fft_size = int(2 ** np.ceil(np.log2(c["N"])))
    draws = R.legacy_draws(c["seed"], fft_size // 2 + 1).astype(np.float32)
    got = simulation.generate_isotropic_noise(R.ISO_MICS, c["N"], c["fs"], type=c["type"], spectrum=c["spectrum"], draws=draws)
    want = G[name + "_out"]
    assert got.shape == want.shape and got.is_contiguous()
    err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(name, "rel err %.3e bound %.3e" % (err, ISO_TOL))
    assert err <= ISO_TOL


def test_gpu_isotropic_in_kernel_draws():
    import torch
    from pykaldi2_amd import simulation
    N, F = 3000, 2049
    draws = simulation.iso_gauss(9, 512, F)
    want = R.gauss_host(9, 512, F)
    err = np.abs(draws.cpu().numpy() - want).max() / np.abs(want).max()
    print("iso_gauss rel err %.3e bound %.3e" % (err, GAUSS_TOL))
    assert err <= GAUSS_TOL
    a = simulation.iso_noise_spectra(R.ISO_MICS, N, 16000, "sph", "hoth", seed=9)
    assert a.shape == (3, F) and a.dtype == torch.complex64
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(simulation.iso_noise_spectra(R.ISO_MICS, N, 16000, "sph", "hoth", draws=draws)))
    x = simulation.generate_isotropic_noise(R.ISO_MICS, N, 16000, "sph", "hoth", seed=9)
    assert torch.equal(x, simulation.generate_isotropic_noise(R.ISO_MICS, N, 16000, "sph", "hoth", seed=9))
    assert not torch.equal(x, simulation.generate_isotropic_noise(R.ISO_MICS, N, 16000, "sph", "hoth", seed=10))
    np.random.seed(3)                # seed=None: one randint of the global generator
    y = simulation.generate_isotropic_noise(R.ISO_MICS, N, 16000, "sph", "hoth")
    rs = np.random.RandomState(3)
    assert torch.equal(y, simulation.generate_isotropic_noise(R.ISO_MICS, N, 16000, "sph", "hoth", seed=int(rs.randint(0, 2 ** 31 - 1))))
    assert np.random.randint(0, 1000) == rs.randint(0, 1000)


def test_gpu_isotropic_large_fft():
    """FFT size 2^18 (a 10 s utterance at 16 kHz needs it): 64 bins of X against the host restatement from the host's own
    draws, the phase tau * w reaching hundreds of radians (an aperture of 4 m); the time-domain output is finite.  Bound:
    X is linear in the draws with weights of modulus 1 / sqrt(P) per direction, so the device's draws (within GAUSS_TOL of
    the host's) and the float32 sum (ISO_TOL) add."""
    import torch
    from pykaldi2_amd import simulation
    N, seed = 1 << 18, 21
    F = N // 2 + 1
    mics = np.array([[0.0, 0.0, 0.0], [4.0, 0.3, 0.1]])
    X = simulation.iso_noise_spectra(mics, N, 16000, "sph", "white", seed=seed).cpu().numpy()
    bins = np.sort(np.concatenate([[0, 1, 2, F - 2, F - 1], np.random.RandomState(0).choice(np.arange(3, F - 2), 59, replace=False)]))
    assert bins.shape[0] == 64
    tau = R.iso_tau(mics, 16000, "sph")
    assert np.abs(tau).max() * np.pi > 500
    z = R.gauss_host(seed, 512, F, counters=np.arange(512)[:, None] * F + bins[None, :])        # (512, 64, 2)
    z = z[..., 0] + 1j * z[..., 1]
    w = 2 * np.pi * bins / N
    want = np.stack([(z * np.exp(-1j * tau[m][:, None] * w[None, :])).sum(axis=0) for m in range(2)]) / np.sqrt(512)
    scale = np.where((bins == 0) | (bins == F - 1), np.sqrt(N), np.sqrt(N / 2))
    want = np.where((bins == 0) | (bins == F - 1), want.real, want) * scale
    err = np.abs(X[:, bins] - want).max() / np.abs(want).max()
    print("2^18 spectra rel err %.3e bound %.3e" % (err, ISO_TOL + GAUSS_TOL))
    assert err <= ISO_TOL + GAUSS_TOL
    x = simulation.generate_isotropic_noise(mics, N, 16000, "sph", "white", seed=seed)
    assert x.shape == (2, N) and bool(torch.isfinite(x).all())
    assert abs(float(x.var()) - 1) < 0.05


@pytest.mark.parametrize("type", ["sph", "cyl"])
def test_gpu_isotropic_field_coherence(type):
    """Two microphones 0.1 m apart, white spectrum, N = 2^16: over 32 bands of K = 1024 bins the band average of
    Re(X0 X1*) / E|X|^2 lies within 5 / sqrt(K) of the quadrature (1 / 512) sum_i cos(tau_i w) (each term has a variance of
    at most 1), and every channel has a variance within 5 % of 1."""
    from pykaldi2_amd import simulation
    N, K = 1 << 16, 1024
    mics = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    X = simulation.iso_noise_spectra(mics, N, 16000, type, "white", seed=5).cpu().numpy().astype(np.complex128)
    f = np.arange(1, N // 2)             # the bins between DC and Nyquist, E|X|^2 = N there: 32 bands of 1023 or 1024
    est = (X[0, f] * np.conj(X[1, f])).real / N
    want = R.iso_coherence(R.iso_tau(mics, 16000, type)[1], 2 * np.pi * f / N)
    nb = 32
    edges = np.linspace(0, f.shape[0], nb + 1).astype(int)
    for b in range(nb):
        sl = slice(edges[b], edges[b + 1])
        k = edges[b + 1] - edges[b]
        assert abs(est[sl].mean() - want[sl].mean()) < 5 / np.sqrt(k), (type, b)
    assert edges[1] - edges[0] in (K - 1, K) and abs(want[:K].mean() - 1) < 0.1 and abs(want[-K:].mean()) < 0.3      # coherent at low, diffuse at high frequencies
    x = simulation.generate_isotropic_noise(mics, N, 16000, type, "white", seed=5).cpu().numpy()
    assert np.abs(x.var(axis=1) - 1).max() < 0.05


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_gpu_simmc_argument_errors():
    import torch
    from pykaldi2_amd import _lib, simulation
    bad = (_lib.Pk2Error, ValueError)
    x = torch.randn(1000, device="cuda")
    rir = torch.randn(3, 64, device="cuda")
    with pytest.raises(bad):
        simulation.Distorter.apply_rir(x, rir, delay=64)                               # delay outside the RIR
    with pytest.raises(bad):
        simulation.Distorter.apply_rir(x, rir.double())                                # not float32
    with pytest.raises(bad):
        simulation._apply_rir_batch([x, x], [rir, torch.randn(2, 64, device="cuda")], None)      # channel mismatch
    with pytest.raises(bad):
        simulation._apply_rir_batch([x, x], [rir], None)                               # a source without a RIR
    sig = torch.randn(3, 1000, device="cuda")
    with pytest.raises(bad):
        simulation.Distorter.add_noise(sig, torch.randn(2, 400, device="cuda"), 5.0)   # channel mismatch
    with pytest.raises(bad):
        simulation.Distorter.add_noise(sig, torch.randn(3, 400, device="cuda"), 5.0, start=700)      # 700 + 400 > 1000
    with pytest.raises(bad):
        simulation.Distorter.add_noise(sig, torch.randn(3, 400, device="cuda"), 5.0, start=201,
                                       noise_position_scheme="repeat_noise")           # tiled to 1200: start <= 200
    with pytest.raises(bad):
        simulation.Distorter.add_noise(sig, torch.randn(3, 400, device="cuda"), 5.0, noise_position_scheme="tile")
    with pytest.raises(bad):
        simulation.Mixer().mix_signals([sig, torch.randn(2, 500, device="cuda")])      # channel mismatch
    with pytest.raises(bad):
        simulation.Mixer().mix_signals([sig, sig], spr=[1.0, 2.0])                     # one SPR per further source
    with pytest.raises(bad):
        simulation.Mixer().mix_signals([sig, sig], signal2=[sig])
    with pytest.raises(bad):
        simulation.MultiSourceSimulator()([x, x], source_rirs=[rir])
    with pytest.raises(NotImplementedError):
        simulation.MultiSourceSimulator()([x, x], source_rirs=[rir, rir], gen_mask=True)
    for kw in (dict(type="cube"), dict(spectrum="pink")):
        with pytest.raises(ValueError):
            simulation.generate_isotropic_noise(R.ISO_MICS, 3000, 16000, **kw)
    with pytest.raises(ValueError):
        simulation.generate_isotropic_noise(R.ISO_MICS, 3000, 22050)
    with pytest.raises(bad):
        simulation.generate_isotropic_noise(R.ISO_MICS, 3000, 16000, draws=np.zeros((512, 2048, 2), np.float32))
    # the library itself refuses what the Python layer would not send
    L = _lib.lib()
    X = torch.zeros(3, 4, 2, device="cuda")
    assert L.pk2_iso_spectra(_lib.ptr(torch.zeros(3, 512, dtype=torch.float64, device="cuda")), None, None, 1, 3, 512, 4,
                             _lib.ptr(X), _lib.stream_ptr()) != 0                      # 4 bins: FFT size 6
    torch.cuda.synchronize()
