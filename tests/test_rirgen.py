"""Image-method RIR generation, host side (no GPU): the reference's argument checks and exceptions, its T60 helpers,
and the online-RIR draws against the reference's own sampling functions (tests/golden/rirgen.npz, written by
tools/gen_golden_rir.py)."""
import numpy as np
import pytest

from pykaldi2_amd import data, rirgen

ROOM = np.array([4.0, 7.0, 3.0]).reshape(3, 1)
SRC = np.array([[1.0], [2.0], [1.5]])
MIC = np.array([[3.0], [5.0], [1.2]])


@pytest.fixture(scope="module")
def G(golden):
    return golden("rirgen")


def test_t60_too_small_for_the_room():
    with pytest.raises(Exception, match="t60 value 0.01 too small for the room"):
        rirgen.xp_rirgen(ROOM, SRC, MIC, t60=0.01)


@pytest.mark.parametrize("beta", [[0.5, 0.5, 0.5, 0.5, 0.5, 1.0], [0.5, 0.0, 0.5, 0.5, 0.5, 0.5], [0.2] * 5 + [-0.1]])
def test_beta_outside_the_open_interval(beta):
    with pytest.raises(Exception, match=r"beta array values should be in the interval \(0,1\)"):
        rirgen.xp_rirgen(ROOM, SRC, MIC, beta=np.array(beta))


@pytest.mark.parametrize("src, mic", [(np.array([[1.0], [7.5], [1.0]]), MIC), (SRC, np.array([[0.0], [1.0], [1.0]])),
                                      (SRC, np.array([[1.0, 2.0], [1.0, 2.0], [1.0, -0.2]]))])
def test_positions_outside_the_room(src, mic):
    with pytest.raises(Exception, match="Room dimensions and source and mic locations are not compatible."):
        rirgen.xp_rirgen(ROOM, src, mic, t60=0.3)


def test_neither_t60_nor_beta():
    with pytest.raises(Exception, match="Either t60 or beta array must be provided"):
        rirgen.xp_rirgen(ROOM, SRC, MIC, t60=None)


def test_method_2_is_not_implemented():
    with pytest.raises(NotImplementedError):
        rirgen.xp_rirgen(ROOM, SRC, MIC, t60=0.3, method=2)


def test_beta_overrides_t60(capsys):
    beta = np.array([0.9, 0.8, 0.7, 0.75, 0.6, 0.85])
    p = rirgen.prepare(ROOM, SRC, MIC, t60=0.01, beta=beta)        # t60 = 0.01 alone would be too small
    assert "Overwriting provided t60 value" in capsys.readouterr().out
    alpha = 1 - beta ** 2
    r = ROOM[:, 0]
    t60 = 24 * np.log(10.0) * np.prod(r) / (340 * 2 * (r[1] * r[2] * (alpha[0] + alpha[1]) + r[0] * r[2] * (alpha[2] + alpha[3])
                                                        + r[0] * r[1] * (alpha[4] + alpha[5])))
    assert p["nsamples"] == int(16000 * t60) and np.array_equal(p["f64"][3:9], beta)


def test_descriptor_follows_the_reference_defaults():
    p = rirgen.prepare(ROOM, SRC, MIC)                                 # t60 = 0.5, c = 340, fs = 16000
    assert p["nsamples"] == 8000 and p["htw"] == min(32, int(3.0 / 10 / 340 * 16000)) == 14 and p["mode"] == 1
    assert rirgen.prepare(ROOM, SRC, MIC, hpfilt=False)["mode"] == 0
    h = rirgen.prepare(ROOM, SRC, MIC, habets_compat=True)
    assert h["htw"] == 64 and h["mode"] == 2
    assert rirgen.prepare(np.array([0.2, 1.5, 1.2]), [0.1, 0.4, 0.5], [0.12, 1.1, 0.7], t60=0.2)["htw"] == 0
    cts = 340 / 16000
    assert np.array_equal(p["f64"][0:3], ROOM[:, 0] / cts)
    assert np.array_equal(p["pos"], np.concatenate([SRC[:, 0], MIC[:, 0]]) / cts)
    for q in range(3):                                                 # never narrower than the reference's lattice rule
        nrefl = int(8000 / (ROOM[q, 0] / cts))
        assert p["half"][q] <= nrefl and 2 * (p["half"][q] + 1) * (ROOM[q, 0] / cts) >= 8000


def test_t60_helpers():
    r = np.array([5.0, 4.0, 3.0])
    V, S = 60.0, 2 * (15.0 + 12.0 + 20.0)
    assert np.isclose(rirgen.t60_to_alpha(r, 0.4), 24 * V * np.log(10) / (343 * S * 0.4), rtol=1e-15)
    assert np.isclose(rirgen.min_t60_of_room(r), 1.1 * 24 * V * np.log(10) / (343 * S), rtol=1e-15)
    assert rirgen.t60_to_alpha(r, rirgen.min_t60_of_room(r)) < 1


def test_online_draws_match_the_reference(G):
    """sample_room, T60 ~ U[0.1, 0.5] raised to min_t60_of_room, mic at the array centre, speech + noise source: the
    reference's functions with the same seed give the same numbers (and so the same draw order)."""
    np.random.seed(int(G["sample_seed"]))
    for k in range(G["sample_rooms"].shape[0]):
        room, t60, mic, src = rirgen.sample_online_room((0.1, 0.5), 2)
        assert np.array_equal(room, G["sample_rooms"][k])
        assert t60 == G["sample_t60"][k] and t60 >= rirgen.min_t60_of_room(room)
        assert np.array_equal(mic, G["sample_mics"][k]) and np.array_equal(src, G["sample_srcs"][k])
        rirgen.prepare(room, src, mic, t60=t60)             # every draw is a valid xp_rirgen call


def test_simulation_pool_online_rir_config():
    on = dict(data_config=dict(simulation_prob=1, use_dir_noise=True, use_reverb=True, online_rir=True), synthetic=True)
    pool = data.SimulationPool.from_config(on)
    assert pool.online_rir and not pool.rirs and pool.sim.use_rir and pool.t60_range == (0.1, 0.5)
    on["data_config"]["t60_range"] = [0.2, 0.3]
    assert data.SimulationPool.from_config(on).t60_range == (0.2, 0.3)
    no_reverb = dict(data_config=dict(simulation_prob=1, use_dir_noise=True, use_reverb=False, online_rir=True), synthetic=True)
    assert not data.SimulationPool.from_config(no_reverb).online_rir
    on["rir_paths"] = [dict(wav="unused.zip")]
    with pytest.warns(UserWarning, match="online_rir"):
        assert data.SimulationPool.from_config(on).online_rir
    off = dict(data_config=dict(simulation_prob=1, use_dir_noise=True, use_reverb=True), synthetic=True)
    pool = data.SimulationPool.from_config(off)
    assert not pool.online_rir and len(pool.rirs) == 16
