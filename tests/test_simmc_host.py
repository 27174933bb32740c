"""Multi-channel / multi-source simulation, host side: the float64 restatement tests/simmc_ref.py against the reference's
own outputs (tests/golden/simulation_mc.npz, written by tools/gen_golden_simmc.py), the numpy Hoth spline of the product
against the reference's scipy one, the host restatement of the device's counter-based normal generator, and the host
halves of the new entry points (draw order, argument errors, array placement)."""
import numpy as np
import pytest

import simmc_ref as R


@pytest.fixture(scope="module")
def G(golden):
    return golden("simulation_mc")


@pytest.mark.parametrize("name", sorted(R.REVERB_CASES))
def test_ref_apply_rir_matches_reference(G, name):
    wav, rir = R.inputs_reverb(name)
    c = R.REVERB_CASES[name]
    assert int(np.argmax(rir[0])) == c["delay"] and int(np.argmax(rir[1])) != c["delay"]      # channel 0 sets the delay
    rv, er = R.apply_rir(wav, rir, get_early_reverb=True)
    assert rv.shape == (c["C"], c["n"])
    assert np.abs(rv - G[name + "_out"]).max() < 1e-12 and np.abs(er - G[name + "_early"]).max() < 1e-12
    cut = min(c["k"], 640 + c["delay"])
    assert (cut == c["k"]) == (name == "rev_b") and (name == "rev_b" or cut % 4 != 0)
    if cut < c["k"]:
        assert np.abs(rv - er).max() > 1e-3       # the early part is not the whole


def test_ref_mixer_matches_reference(G):
    c = R.MIXER_CASE
    sig, sig2 = R.inputs_mixer()
    np.random.seed(c["draw_seed"])
    starts = R.draw_mix_starts(c["lengths"])
    assert starts == G["mix_starts"].tolist() and starts[0] == 0 and starts[2] == 0 and starts[1] > 0
    mixed, scale, pos2 = R.mix(sig, c["spr"], starts, sig2)
    assert np.abs(scale - G["mix_scale"]).max() < 1e-12 and scale[0] == 1.0
    assert np.abs(mixed - G["mix_out"]).max() < 1e-12
    assert np.abs(sum(pos2) - G["mix_out2"]).max() < 1e-12


@pytest.mark.parametrize("name", sorted(R.NOISE_CASES))
def test_ref_add_noise_matches_reference(G, name):
    c = R.NOISE_CASES[name]
    sig, nz = R.inputs_noise(name)
    np.random.seed(c["draw_seed"])
    before = np.random.get_state()[2]
    start = R.draw_noise_start(c["n"], c["m"], c["scheme"])
    assert start == int(G[name + "_start"])
    if name.endswith("equal"):
        assert start == 0 and np.random.get_state()[2] == before      # no draw
    got = R.add_noise(sig, nz, c["snr"], start, c["scheme"])
    assert np.abs(got - G[name + "_out"]).max() < 1e-12


@pytest.mark.parametrize("name", sorted(R.ISO_CASES))
def test_ref_isotropic_noise_matches_reference(G, name):
    c = R.ISO_CASES[name]
    fft_size = int(2 ** np.ceil(np.log2(c["N"])))
    got = R.iso_noise(R.ISO_MICS, c["N"], c["fs"], c["type"], c["spectrum"], R.legacy_draws(c["seed"], fft_size // 2 + 1))
    want = G[name + "_out"]
    assert got.shape == want.shape == (3, c["N"])
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("fs,fft_size", [(16000, 4096), (16000, 2048), (8000, 2048)])
def test_numpy_hoth_spline_matches_reference(G, fs, fft_size):
    from pykaldi2_amd import simulation
    want = G["hoth_%d_%d" % (fs, fft_size)]
    got = simulation._get_hoth_mag(fs, fft_size)
    assert got.shape == want.shape and got[0] == 0.0
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(R.hoth_mag(fs, fft_size) - want).max() == 0.0


def test_direction_samplers_match_restatement():
    from pykaldi2_amd import simulation
    assert np.array_equal(simulation._sample_sphere(512), R.sample_sphere())
    assert np.array_equal(simulation._sample_circle(512), R.sample_circle())
    assert np.abs(np.linalg.norm(R.sample_sphere(), axis=0) - 1).max() < 1e-12


def test_counter_generator_restatement_is_standard_normal():
    n = 1 << 20
    z = R.gauss_host(12345, 512, n // 1024)             # 2^19 pairs = 2^20 draws
    assert z.shape == (512, n // 1024, 2)
    z = z.reshape(-1)
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 / np.sqrt(n)
    assert abs(np.mean(z[0::2] * z[1::2])) < 5 / np.sqrt(n / 2)       # real and imaginary parts are uncorrelated
    # a pure function of (seed, counter): a subset of counters gives the same values; another seed does not
    idx = np.array([0, 7, 512 * 1024 - 1])
    assert np.array_equal(R.gauss_host(12345, 512, n // 1024, counters=idx), z.reshape(-1, 2)[idx])
    assert not np.array_equal(R.gauss_host(12346, 512, n // 1024, counters=idx), z.reshape(-1, 2)[idx])
    # the float32 steps of the kernel stay at float32 accuracy, also where u1 is within 2^-24 of 1
    z32 = R.gauss_host(12345, 512, 64, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - R.gauss_host(12345, 512, 64)).max() < 2e-6


def test_isotropic_noise_argument_errors_need_no_gpu():
    from pykaldi2_amd import simulation
    mics = R.ISO_MICS
    for kw in (dict(samp_rate=44100), dict(type="cube"), dict(spectrum="pink")):
        args = dict(dict(samp_rate=16000, type="sph", spectrum="white"), **kw)
        with pytest.raises(ValueError):
            simulation.generate_isotropic_noise(mics, 3000, args["samp_rate"], type=args["type"], spectrum=args["spectrum"])
    with pytest.raises(ValueError):
        simulation.generate_isotropic_noise(mics[:, :2], 3000, 16000)       # not (C, 3)
    with pytest.raises(ValueError):
        simulation.Distorter.add_noise(None, None, 5.0, noise_position_scheme="loop_noise")
    with pytest.raises(NotImplementedError):
        simulation.MultiSourceSimulator()([None, None], gen_mask=True)
    fft_size, tau, g = simulation._iso_setup(mics, 3000, 16000, "cyl", "hoth")
    assert fft_size == 4096 and g.shape == (2049,) and np.abs(tau - R.iso_tau(mics, 16000, "cyl")).max() < 1e-12
    assert not tau[0].any()


def test_sample_array_is_the_centre_draw_plus_offsets():
    from pykaldi2_amd import rirgen
    geo = np.array([[0.0425 * np.cos(a), 0.0425 * np.sin(a), 0.0] for a in np.arange(6) * np.pi / 3] + [[0.0, 0.0, 0.0]]).T
    room = np.array([6.0, 5.0, 3.0])
    np.random.seed(5)
    want = rirgen.sample_array_center(room)
    np.random.seed(5)
    ctr, mic = rirgen.sample_array(room, geo)
    assert np.array_equal(ctr, want) and mic.shape == (3, 7) and np.array_equal(mic, want + geo)
    # sample_online_room: the default call draws what it drew before; with an array the same draws place 7 microphones
    np.random.seed(6)
    room0, t0, mic0, src0 = rirgen.sample_online_room()
    np.random.seed(6)
    room1, t1, mic1, src1 = rirgen.sample_online_room(mic_positions=geo)
    assert np.array_equal(room0, room1) and t0 == t1 and np.array_equal(src0, src1)
    assert mic0.shape == (3, 1) and np.array_equal(mic1, mic0 + geo)
    with pytest.raises(ValueError):
        rirgen.sample_array(room, geo.T)
