"""The beamformer without a GPU: properties of the float64 restatement (tests/beamform_ref.py), the conditions the GPU
tests rely on, the data_config key `beamform`, and the argument checks of the three ABI entries, which run before the device
is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_ref as R  # noqa: E402

from pykaldi2_amd import _lib, beamform  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pd(r, F, Cn):
    a = r.standard_normal((F, Cn, Cn + 2)) + 1j * r.standard_normal((F, Cn, Cn + 2))
    return a @ a.conj().transpose(0, 2, 1) + 0.1 * np.eye(Cn)


def test_constants_match_the_restatement_and_the_header():
    assert beamform.FRAMES_PER_PART == _lib.BF_FRAMES_PER_PART == R.P == 32
    assert (beamform.MAX_CHANNELS, beamform.MAX_MASKS, _lib.BF_REF_SNR) == (8, 4, -1)
    hdr = open(os.path.join(ROOT, "include", "pk2hip.h")).read()
    for line in ("#define PK2_BF_MAX_CHANNELS 8\n", "#define PK2_BF_MAX_MASKS 4\n", "#define PK2_BF_FRAMES_PER_PART 32\n",
                 "#define PK2_BF_REF_SNR (-1)\n"):
        assert line in hdr


@pytest.mark.parametrize("Cn,ref", [(1, 0), (2, 1), (4, 0), (8, 5)])
def test_distortionless_in_soudens_form(Cn, ref):
    """Phi_s = sigma d d^H and any positive-definite Phi_n: w^H d = d_r (the loaded Phi_n' is just another positive-definite
    matrix, so the default loading stays on)."""
    r = np.random.RandomState(Cn)
    F = 9
    d = r.standard_normal((F, Cn)) + 1j * r.standard_normal((F, Cn))
    phi_s = 2.5 * d[:, :, None] * d.conj()[:, None, :]
    w, got = R.mvdr_weights(phi_s, _pd(r, F, Cn), ref)
    assert got == ref
    wd = np.einsum("fc,fc->f", w.conj(), d)
    # w = Pn^-1 d d^H e_r sigma / (sigma d^H Pn^-1 d) = Pn^-1 d conj(d_r) / (d^H Pn^-1 d), so w^H d = d_r
    assert np.abs(wd - d[:, ref]).max() <= 1e-12 * np.abs(d).max()


@pytest.mark.parametrize("name", ["c2_f33_n31_k2", "c8_f17_n33_comp", "c3_f257_n32_k4"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_covariances_are_hermitian_with_a_real_diagonal(name, dtype):
    Y, m = R.case_inputs(name)
    phi = R.covariance(Y, m, R.CASES[name][4], dtype)
    assert phi.shape == ((2 if R.CASES[name][4] else R.CASES[name][3]), R.CASES[name][1], R.CASES[name][0], R.CASES[name][0])
    assert np.array_equal(phi, phi.conj().transpose(0, 1, 3, 2))
    assert not np.diagonal(phi, axis1=-2, axis2=-1).imag.any()
    assert (np.diagonal(phi, axis1=-2, axis2=-1).real >= 0).all()


def test_complement_is_the_covariance_of_one_minus_the_mask():
    Y, m = R.case_inputs("c3_f33_n200_comp")
    both = R.covariance(Y, m, True)
    assert np.array_equal(both[0], R.covariance(Y, m)[0])
    assert np.array_equal(both[1], R.covariance(Y, 1.0 - m.astype(np.float64))[0])


def test_an_empty_speech_mask_passes_the_reference_channel():
    Y, m = R.case_inputs("c2_f257_n98_zero_bins")
    phi = R.covariance(Y, m, True)
    empty = ~m[0].any(axis=0)
    assert empty.sum() >= 52 and not phi[0][empty].any()
    for ref in (0, 1):
        w, _ = R.mvdr_weights(phi[0], phi[1], ref)
        assert np.array_equal(w[empty], np.tile(np.eye(2)[ref], (empty.sum(), 1)))
        assert np.abs(w[~empty] - np.eye(2)[ref]).max(axis=1).min() > 0


def test_scaling_either_mask_leaves_the_weights_unchanged():
    Y, m = R.case_inputs("c8_f257_n98_k2")
    w, _ = R.mvdr_weights(*R.covariance(Y, m), ref=3)
    for a, b in ((0.25, 1.0), (1.0, 0.125), (0.5, 0.03125)):
        scaled = np.stack([a * m[0], b * m[1]])
        w2, _ = R.mvdr_weights(*R.covariance(Y, scaled), ref=3)
        assert np.abs(w2 - w).max() <= 1e-9 * np.abs(w).max()


def test_snr_reference_is_the_argmax_and_ties_go_to_the_lowest_channel():
    Y, m = R.case_inputs("c3_f33_n200_comp")
    phi = R.covariance(Y, m, True)
    snr = R.snr_per_channel(phi[0], phi[1])
    w, r = R.mvdr_weights(phi[0], phi[1], "snr")
    assert r == int(np.argmax(snr)) and np.array_equal(w, R.mvdr_weights(phi[0], phi[1], r)[0])
    tie_s, tie_n = R.tie_covariances()
    snr = R.snr_per_channel(tie_s, tie_n)
    assert snr[0] == snr[1] == snr[2] == snr.max()
    assert R.mvdr_weights(tie_s, tie_n, "snr")[1] == 0


@pytest.mark.parametrize("name", R.SNR_CASES)
def test_condition_the_best_channel_leads_by_one_percent(name):
    Y, m = R.case_inputs(name)
    phi = R.covariance(Y, m, R.CASES[name][4])
    snr = np.sort(R.snr_per_channel(phi[0], phi[1]))
    assert snr[-1] >= 1.01 * snr[-2] > 0


def test_condition_the_scene_gains_six_decibels():
    wav, target, mask = R.scene()
    assert wav.shape == (4, 16000)
    y, _, _, _ = R.beamform(wav, mask)
    assert R.scene_gain(y, wav, target) >= 6.0


def test_float32_mode_stays_close_to_float64():
    Y, m = R.case_inputs("c8_f257_n98_k2")
    a, b = R.covariance(Y, m), R.covariance(Y, m, dtype=np.float32)
    assert b.dtype == np.complex64 and 0 < np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


# ---------------------------------------------------------------------------------------------------------------------
# data_config `beamform`
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(value, **dc):
    base = dict(online_rir=True, use_reverb=True, simulation_prob=0.5)
    base.update(dc)
    return {"data_config": dict(base, beamform=value)}


def test_config_accepted_forms():
    assert beamform.beamform_config(_cfg(True)) == dict(n_mics=7, radius=0.0425, ref=0, diag_load=0.001)
    assert beamform.beamform_config(_cfg({"n_mics": 4, "ref": "snr"})) == dict(n_mics=4, radius=0.0425, ref="snr", diag_load=0.001)
    assert beamform.beamform_config(_cfg({})) == beamform.CONFIG_DEFAULTS
    for absent in ({}, {"data_config": {}}, _cfg(False), _cfg(None), {"data_config": {"beamform": False, "simulation_prob": 0}}):
        assert beamform.beamform_config(absent) is None


@pytest.mark.parametrize("dc,word", [(dict(online_rir=False), "online_rir"), (dict(use_reverb=False), "use_reverb"),
                                     (dict(simulation_prob=0), "simulation_prob")])
def test_config_names_the_missing_key(dc, word):
    with pytest.raises(ValueError, match=word):
        beamform.beamform_config(_cfg(True, **dc))
    cfg = _cfg(True, **dc)
    for k in dc:
        del cfg["data_config"][k]
    with pytest.raises(ValueError, match=word):
        beamform.beamform_config(cfg)


@pytest.mark.parametrize("value,word", [({"n_mics": 9}, "n_mics"), ({"n_mics": 0}, "n_mics"), ({"n_mics": 2.5}, "n_mics"),
                                        ({"radius": 0}, "radius"), ({"radius": "wide"}, "radius"), ({"ref": 7}, "ref"),
                                        ({"ref": -1}, "ref"), ({"ref": "best"}, "ref"), ({"diag_load": -1}, "diag_load"),
                                        ({"diag_load": float("nan")}, "diag_load"), ({"mics": 4}, "mics"), (3, "mapping")])
def test_config_bad_values_name_their_key(value, word):
    with pytest.raises(ValueError, match=word):
        beamform.beamform_config(_cfg(value))


def test_config_start_up_exit_is_one_line():
    code = ("import sys; sys.path.insert(0, %r); from pykaldi2_amd import beamform; "
            "beamform.require_beamform_config({'data_config': {'beamform': True, 'use_reverb': True, 'simulation_prob': 1}}, 'prog')"
            % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "online_rir" in out.stderr and "Traceback" not in out.stderr


def test_array_geometry():
    g = beamform.array_geometry(7, 0.0425)
    assert g.shape == (3, 7) and not g[:, 0].any() and not g[2].any()
    assert np.allclose(np.hypot(g[0, 1:], g[1, 1:]), 0.0425)
    assert np.allclose(np.hypot(*(g[:2, 1] - g[:2, 2])), 0.0425)        # a hexagon's side is its radius
    g4 = beamform.array_geometry(4, 0.05)
    assert g4.shape == (3, 4) and np.allclose(np.hypot(g4[0], g4[1]), 0.05) and np.allclose(g4[:2].sum(axis=1), 0)


def test_pool_without_the_key_has_no_beamformer():
    from pykaldi2_amd import data
    cfg = {"synthetic": True, "data_config": dict(online_rir=True, use_reverb=True, use_dir_noise=True, simulation_prob=1.0)}
    assert data.SimulationPool.from_config(cfg).beamform is None
    with pytest.raises(ValueError, match="online_rir"):
        data.SimulationPool.from_config({"synthetic": True, "data_config": dict(use_reverb=True, simulation_prob=1.0, beamform=True)})


# ---------------------------------------------------------------------------------------------------------------------
# the ABI refuses bad arguments before it touches the device
# ---------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.lib().pk2_last_error().lower()


def test_bad_abi_arguments_fail_loudly():
    L = _lib.lib()
    one = (C.c_void_p * 4)(8, 8, 8, 8)           # never dereferenced: every call below is refused on the host
    frames = (C.c_int32 * 1)(5)
    work = C.c_void_p(8)
    assert L.pk2_bf_cov(None, one, frames, 1, 2, 17, 1, 0, work, 1 << 20, work, None) < 0 and b"null" in _err()
    assert L.pk2_bf_cov(one, one, frames, 0, 2, 17, 1, 0, work, 1 << 20, work, None) < 0 and b"no utterance" in _err()
    assert L.pk2_bf_cov(one, one, frames, 1, 9, 17, 1, 0, work, 1 << 20, work, None) < 0 and b"channels" in _err()
    assert L.pk2_bf_cov(one, one, frames, 1, 2, 0, 1, 0, work, 1 << 20, work, None) < 0 and b"bins" in _err()
    assert L.pk2_bf_cov(one, one, frames, 1, 2, 17, 5, 0, work, 1 << 20, work, None) < 0 and b"masks" in _err()
    assert L.pk2_bf_cov(one, one, frames, 1, 2, 17, 2, 1, work, 1 << 20, work, None) < 0 and b"complement" in _err()
    assert L.pk2_bf_cov(one, one, (C.c_int32 * 1)(0), 1, 2, 17, 1, 0, work, 1 << 20, work, None) < 0 and b"frames" in _err()
    assert L.pk2_bf_cov(one, one, frames, 1, 2, 17, 1, 0, work, 16, work, None) < 0 and b"workspace" in _err()
    with pytest.raises(_lib.Pk2Error):
        _lib.check(L.pk2_bf_cov(one, one, None, 1, 2, 17, 1, 0, work, 1 << 20, work, None))
    need = L.pk2_bf_workspace_bytes(frames, 1, 2, 17, 1, 0)
    assert need >= 1 * 1 * 7 * 17 * 4 and L.pk2_bf_workspace_bytes(None, 1, 2, 17, 1, 0) > 0
    assert L.pk2_bf_workspace_bytes(frames, 1, 9, 17, 1, 0) == 0 and L.pk2_bf_workspace_bytes(frames, 1, 2, 17, 2, 1) == 0

    big = 1 << 24
    assert L.pk2_bf_mvdr_weights(one, None, 1, 2, 17, 0, 1e-3, work, big, work, work, work, None) < 0 and b"null" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, 2, 1e-3, work, big, work, work, work, None) < 0 and b"ref" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, -2, 1e-3, work, big, work, work, work, None) < 0 and b"ref" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, 0, -1.0, work, big, work, work, work, None) < 0 and b"diag_load" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, 0, float("nan"), work, big, work, work, work, None) < 0
    assert L.pk2_bf_mvdr_weights(one, one, 1, 9, 17, 0, 1e-3, work, big, work, work, work, None) < 0 and b"channels" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, 0, 1e-3, work, 8, work, work, work, None) < 0 and b"workspace" in _err()
    assert L.pk2_bf_mvdr_weights(one, one, 1, 2, 17, 0, 1e-3, work, big, work, None, work, None) < 0 and b"null" in _err()

    assert L.pk2_bf_apply(one, one, frames, 1, 2, 17, None, None) < 0 and b"null" in _err()
    assert L.pk2_bf_apply(one, one, frames, 1, 0, 17, one, None) < 0 and b"channels" in _err()
    assert L.pk2_bf_apply(one, one, (C.c_int32 * 1)(-3), 1, 2, 17, one, None) < 0 and b"frames" in _err()
    assert L.pk2_bf_apply(one, (C.c_void_p * 1)(None), frames, 1, 2, 17, one, None) < 0 and b"null" in _err()


def test_python_argument_errors_that_need_no_gpu():
    with pytest.raises(ValueError, match="ref"):
        beamform.MaskBeamformer(None, ref="loudest")
    with pytest.raises(ValueError, match="ref"):
        beamform.MaskBeamformer(None, ref=-1)
    with pytest.raises(ValueError, match="diag_load"):
        beamform.MaskBeamformer(None, diag_load=-0.5)
