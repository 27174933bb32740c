"""The cGMM mask estimator without a GPU: properties of the float64 restatement (tests/cgmm_ref.py), the conditions the GPU
tests rely on (the float32 mode's error on their cases, the purity margins), the data_config keys `beamform: {mask,
cgmm_iterations}`, and the argument checks of the ABI entries, which run before the device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgmm_ref as R  # noqa: E402

from pykaldi2_amd import _lib, beamform, cgmm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = [n for n in R.CASES if R.CASES[n][4] == "plain"]
GUIDED = [n for n in R.CASES if R.CASES[n][4] == "guided"]


def test_constants_match_the_restatement_and_the_header():
    assert beamform.FRAMES_PER_PART == R.P == 32
    assert (cgmm.MAX_CHANNELS, cgmm.MAX_CLASSES, cgmm.MAX_ITERS) == (8, 4, 32)
    assert "#define PK2_CGMM_MAX_ITERS 32\n" in open(os.path.join(ROOT, "include", "pk2hip.h")).read()


@pytest.mark.parametrize("name", ["c2_f33_n31", "c7_f33_n33", "c8_f257_n98"])
def test_the_likelihood_never_decreases(name):
    """diag_load = 0 (only the 1e-10 floor is added), no silent frame: every step is an exact EM step"""
    Y, _, _ = R.case_inputs(name)
    ll = R.em(Y, 10, diag_load=0.0)["ll"]
    print(name, "LL", ll)
    assert (np.diff(ll) >= -1e-9 * np.abs(ll[1:])).all()


@pytest.mark.parametrize("name", ["c2_f33_n31", "c7_f33_n33", "c3_f257_n32"])
def test_the_new_covariance_has_trace_C_in_the_old_metric(name):
    """tr(R_old'^-1 R_new) = sum_t lam (y^H R_old'^-1 y) / phi / sum_t lam = C, because phi = y^H R_old'^-1 y / C"""
    Y, _, _ = R.case_inputs(name)
    Cn = Y.shape[0]
    Rk, la = R.init_state(Y)
    Li, b, bad = R.factor(Rk, la, 0.0)
    assert not bad.any()
    lam, phi, _ = R.posteriors(Y, Li, b, bad)
    assert (phi > 1e-10).all()
    Rn, _ = R.update(Y, lam, phi)
    inv_old = np.einsum("kfji,kfjl->kfil", Li.conj(), Li)          # L^-H L^-1
    tr = np.einsum("kfij,kfji->kf", inv_old, Rn)
    assert np.abs(tr - Cn).max() <= 1e-9 * Cn


@pytest.mark.parametrize("name", ["c3_f257_n32", "c3_f33_n200_k3", "c8_f17_n98_k4"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_masks_sum_to_one_where_a_class_is_active(name, dtype):
    Y, init, act = R.case_inputs(name)
    out = R.em(Y, 3, init, act, dtype=dtype)
    m = out["masks"]
    live = np.ones(Y.shape[1], bool) if act is None else (act > 0).any(axis=0)
    assert np.abs(m[:, live].sum(axis=0) - 1).max() <= (1e-6 if dtype == np.float32 else 1e-12)
    assert not m[:, ~live].any() and (m >= 0).all()
    assert np.array_equal(out["R"], out["R"].conj().transpose(0, 1, 3, 2))
    assert not np.diagonal(out["R"], axis1=-2, axis2=-1).imag.any()


def test_one_channel_returns_alpha():
    """C = 1: every class sees phi R = |y|^2, so the posteriors are the priors, whatever the start"""
    Y, _, _ = R.case_inputs("c1_f33_n98")
    out = R.em(Y, 4, order="keep")
    assert np.abs(out["masks"] - 0.5).max() <= 1e-12
    r = np.random.RandomState(0)
    init = r.uniform(0.1, 1, (3,) + Y.shape[1:])
    init /= init.sum(axis=0)
    out = R.em(Y, 2, init.astype(np.float32))
    assert np.abs(out["masks"] - np.exp(out["la"])[:, None, :]).max() <= 1e-9


@pytest.mark.parametrize("Cn", [4, 7])
def test_a_source_in_white_noise_is_found(Cn):
    """A rank-one source in white noise at 10 dB, N = 300, F = 9, on 35 % of the points: the share of points that
    lam_0 > 1/2 classifies like the ideal mask, and no bin swapped.  Measured: 0.919 .. 0.929 (C = 4), 0.948 .. 0.956
    (C = 7) over the three seeds."""
    for seed in (1, 2, 3):
        Y, on = R.scene(Cn, seed)
        out = R.em(Y, 10)
        share = ((out["masks"][0] > 0.5) == on).mean(axis=0)
        p = R.purity(out["R"])
        print("C %d seed %d: share %.3f (per bin %.3f .. %.3f), swapped %d" % (Cn, seed, share.mean(), share.min(), share.max(),
                                                                                  out["swapped"].sum()))
        assert share.mean() >= 0.85
        assert (p[0] > p[1]).all()


def test_a_swapped_start_comes_back_in_the_purity_order():
    Y, on = R.scene(4, 5)
    ideal = np.stack([on, ~on]).astype(np.float32) * 0.9 + 0.05
    keep = R.em(Y, 10, ideal, order="keep")
    swapped = R.em(Y, 10, ideal[::-1].copy(), order="keep")
    assert ((swapped["masks"][1] > 0.5) == on).mean() >= 0.85           # the source stays where the start put it
    back = R.em(Y, 10, ideal[::-1].copy(), order="purity")
    p = R.purity(back["R"])
    assert back["swapped"].all() and (p[0] >= p[1]).all()
    assert np.abs(back["masks"] - keep["masks"]).max() <= 1e-6
    with pytest.raises(ValueError, match="two classes"):
        R.em(Y, 1, np.ones((3,) + on.shape, np.float32) / 3, order="purity")


def test_a_tie_keeps_the_order():
    eye = np.tile(np.eye(3, dtype=np.complex128), (2, 5, 1, 1))
    lam = np.arange(2 * 4 * 5, dtype=np.float64).reshape(2, 4, 5)
    got = R.reorder(lam, eye, np.zeros((2, 5)))
    assert not got[3].any() and np.array_equal(got[0], lam)


def test_an_inactive_class_gets_a_zero_mask():
    Y, init, act = R.case_inputs("c3_f33_n200_k3")
    act = act.copy()
    act[1] = 0
    m = R.em(Y, 3, init, act)["masks"]
    assert not m[1].any()
    live = (act > 0).any(axis=0)
    assert np.abs(m[:, live].sum(axis=0) - 1).max() <= 1e-12 and not m[:, ~live].any()


def test_a_bad_bin_gets_uniform_masks_and_raises_the_flag():
    Y, _, _ = R.case_inputs("c2_f33_n31")
    Y = Y.copy()
    Y[1, 4, 7] = np.nan
    out = R.em(Y, 2)
    assert out["nonfinite"] and (out["masks"][:, :, 7] == 0.5).all()
    keep = np.arange(Y.shape[2]) != 7
    clean = R.em(R.case_inputs("c2_f33_n31")[0], 2)
    assert not clean["nonfinite"] and np.array_equal(out["masks"][:, :, keep], clean["masks"][:, :, keep])


def test_float32_mode_stays_close_on_the_gpu_cases():
    """The GPU test's tolerances are 4 x these (tests/test_gpu_cgmm.py); every one below 1e-3 over 10 iterations"""
    worst = {}
    for name in list(R.CASES) + R.RAGGED:
        e = R.float32_errors(name)
        print(name, " ".join("%s %.2e" % kv for kv in sorted(e.items())))
        assert max(e.values()) < 1e-3, name
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest:", " ".join("%s %.2e" % kv for kv in sorted(worst.items())))


def test_the_purities_of_the_gpu_cases_are_well_apart():
    """The class order on the device is compared with the restatement's on bins whose purities differ by >= 1 % there:
    that must be most bins of the cases, and both orders must occur."""
    seen = set()
    for name in PLAIN + R.RAGGED:
        if R._shape(name)[0] == 1:
            continue                                  # C = 1: both purities are 1
        Y, _, _ = R.case_inputs(name)
        out = R.em(Y, 10, order="keep")
        p = R.purity(out["R"])
        clear = np.abs(p[1] - p[0]) >= 0.01 * np.maximum(p[0], p[1])
        seen.update((p[1] > p[0])[clear].tolist())
        assert clear.mean() >= 0.9, name
    assert seen == {False, True}


# ---------------------------------------------------------------------------------------------------------------------
# data_config `beamform: {mask, cgmm_iterations}`
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(value):
    return {"data_config": dict(online_rir=True, use_reverb=True, simulation_prob=0.5, beamform=value)}


def test_config_keys():
    assert cgmm.cgmm_config(True) == cgmm.cgmm_config({}) == ("ideal", 10)
    assert cgmm.cgmm_config({"mask": "cgmm", "cgmm_iterations": 4}) == ("cgmm", 4)
    # the keys appear in the beamformer's configuration only when they are given: without them it is what it was
    assert beamform.beamform_config(_cfg({"n_mics": 4})) == dict(n_mics=4, radius=0.0425, ref=0, diag_load=0.001)
    got = beamform.beamform_config(_cfg({"n_mics": 4, "mask": "cgmm"}))
    assert got == dict(n_mics=4, radius=0.0425, ref=0, diag_load=0.001, mask="cgmm", cgmm_iterations=10)
    assert beamform.beamform_config(_cfg({"cgmm_iterations": 3}))["mask"] == "ideal"


@pytest.mark.parametrize("value,word", [({"mask": "oracle"}, "mask"), ({"mask": True}, "mask"), ({"mask": "cgmm", "cgmm_iterations": 0},
                                                                                                  "cgmm_iterations"),
                                        ({"cgmm_iterations": 33}, "cgmm_iterations"), ({"cgmm_iterations": 2.5}, "cgmm_iterations"),
                                        ({"cgmm_iterations": True}, "cgmm_iterations"), ({"masks": "cgmm"}, "masks")])
def test_config_bad_values_name_their_key(value, word):
    with pytest.raises(ValueError, match=word):
        beamform.beamform_config(_cfg(value))


def test_pool_takes_the_estimator_only_with_the_key():
    from pykaldi2_amd import data
    dc = dict(online_rir=True, use_reverb=True, use_dir_noise=True, simulation_prob=1.0)
    pool = data.SimulationPool.from_config({"synthetic": True, "data_config": dict(dc, beamform={"n_mics": 4})})
    assert pool.cgmm is None
    pool = data.SimulationPool.from_config({"synthetic": True, "data_config": dict(dc, beamform={"n_mics": 4, "mask": "ideal"})})
    assert pool.cgmm is None
    pool = data.SimulationPool.from_config({"synthetic": True,
                                            "data_config": dict(dc, beamform={"mask": "cgmm", "cgmm_iterations": 5})})
    assert isinstance(pool.cgmm, cgmm.CgmmMaskEstimator) and pool.cgmm.iterations == 5


def test_decode_wav_channels():
    import io
    import wave
    from pykaldi2_amd import data
    pcm = (np.arange(3 * 50).reshape(50, 3) * 100 - 7000).astype("<i2")
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(3)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    x, sr = data.decode_wav_channels(buf.getvalue())
    assert sr == 16000 and x.shape == (3, 50) and x.dtype == np.float32 and x.flags.c_contiguous
    assert np.array_equal(x, pcm.T.astype(np.float32) / 32768.0)
    assert np.array_equal(data.decode_wav(buf.getvalue())[0], x[0])


# ---------------------------------------------------------------------------------------------------------------------
# arguments: the ABI refuses before it touches the device, the Python layer before it launches
# ---------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.lib().pk2_last_error().lower()


def test_bad_abi_arguments_fail_loudly():
    L = _lib.lib()
    one = (C.c_void_p * 4)(8, 8, 8, 8)           # never dereferenced: every call below is refused on the host
    frames = (C.c_int32 * 1)(5)
    w = C.c_void_p(8)
    big = 1 << 26

    def run(spec=one, init=None, act=None, fr=frames, B=1, Cn=2, F=17, K=2, iters=3, load=1e-3, purity=1, work=w, nbytes=big,
            masks=one, Rp=w, la=w, ll=w, flag=w):
        return L.pk2_cgmm(spec, init, act, fr, B, Cn, F, K, iters, load, purity, work, nbytes, masks, Rp, la, ll, flag, None)
    assert run(spec=None) < 0 and b"null" in _err()
    assert run(B=0) < 0 and b"no utterance" in _err()
    assert run(Cn=9) < 0 and b"channels" in _err()
    assert run(Cn=0) < 0 and b"channels" in _err()
    assert run(F=0) < 0 and b"bins" in _err()
    assert run(K=1) < 0 and b"classes" in _err()
    assert run(K=5, init=one) < 0 and b"classes" in _err()
    assert run(K=3) < 0 and b"initial masks" in _err()
    assert run(K=3, init=one, purity=1) < 0 and b"purity" in _err()
    assert run(iters=0) < 0 and b"iterations" in _err()
    assert run(iters=33) < 0 and b"iterations" in _err()
    assert run(load=-1.0) < 0 and b"diag_load" in _err()
    assert run(load=float("nan")) < 0 and b"diag_load" in _err()
    assert run(fr=None) < 0 and b"frames" in _err()
    assert run(fr=(C.c_int32 * 1)(0)) < 0 and b"frames" in _err()
    assert run(nbytes=16) < 0 and b"workspace" in _err()
    assert run(masks=None) < 0 and b"null" in _err()
    assert run(masks=(C.c_void_p * 1)(None)) < 0 and b"null" in _err()
    assert run(act=(C.c_void_p * 1)(None)) < 0 and b"null" in _err()
    assert run(ll=None) < 0 and b"null" in _err()
    assert run(flag=None) < 0 and b"null" in _err()
    with pytest.raises(_lib.Pk2Error):
        _lib.check(run(work=None))

    need = L.pk2_cgmm_workspace_bytes(frames, 1, 2, 17, 2)
    assert need >= 2 * (5 * 2 * 17 * 4) + 2 * 7 * 17 * 4
    assert L.pk2_cgmm_workspace_bytes(None, 1, 2, 17, 2) == 0 and L.pk2_cgmm_workspace_bytes(frames, 1, 9, 17, 2) == 0
    assert L.pk2_cgmm_workspace_bytes(frames, 1, 2, 17, 1) == 0 and L.pk2_cgmm_workspace_bytes(frames, 1, 2, 17, 5) == 0
    assert L.pk2_cgmm_workspace_bytes((C.c_int32 * 1)(0), 1, 2, 17, 2) == 0

    assert L.pk2_cgmm_init(one, None, None, frames, 1, 2, 17, 3, w, big, w, w, None) < 0 and b"initial masks" in _err()
    assert L.pk2_cgmm_init(one, None, None, frames, 1, 2, 17, 2, w, 16, w, w, None) < 0 and b"workspace" in _err()
    assert L.pk2_cgmm_init(one, None, None, frames, 1, 2, 17, 2, w, big, None, w, None) < 0 and b"null" in _err()
    assert L.pk2_cgmm_factor(w, w, 1, 2, 17, 2, -1.0, w, w, w, w, None) < 0 and b"diag_load" in _err()
    assert L.pk2_cgmm_factor(w, None, 1, 2, 17, 2, 1e-3, w, w, w, w, None) < 0 and b"null" in _err()
    assert L.pk2_cgmm_factor(w, w, 1, 9, 17, 2, 1e-3, w, w, w, w, None) < 0 and b"channels" in _err()
    assert L.pk2_cgmm_posteriors(one, None, frames, 1, 2, 17, 2, w, w, None, w, big, one, one, w, None) < 0 and b"null" in _err()
    assert L.pk2_cgmm_posteriors(one, None, frames, 1, 2, 17, 2, w, w, w, w, big, one, None, w, None) < 0 and b"null" in _err()
    assert L.pk2_cgmm_posteriors(one, None, frames, 1, 2, 17, 2, w, w, w, w, 16, one, one, w, None) < 0 and b"workspace" in _err()
    assert L.pk2_cgmm_update(one, one, None, None, frames, 1, 2, 17, 2, w, big, w, w, None) < 0 and b"null" in _err()
    assert L.pk2_cgmm_update(one, one, one, None, frames, 1, 2, 17, 5, w, big, w, w, None) < 0 and b"classes" in _err()
    assert L.pk2_cgmm_update(one, one, one, None, (C.c_int32 * 1)(-2), 1, 2, 17, 2, w, big, w, w, None) < 0 and b"frames" in _err()


def test_python_argument_errors_that_need_no_gpu():
    with pytest.raises(ValueError, match="iterations"):
        cgmm.CgmmMaskEstimator(None, iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        cgmm.CgmmMaskEstimator(None, iterations=33)
    with pytest.raises(ValueError, match="diag_load"):
        cgmm.CgmmMaskEstimator(None, diag_load=-1)
    with pytest.raises(ValueError, match="kind"):
        cgmm.ArrayFrontEnd("none")
    with pytest.raises(ValueError, match="mask_estimator"):
        beamform.MaskBeamformer(None, mask_estimator=object())
    with pytest.raises(ValueError, match="no speech mask"):
        beamform.MaskBeamformer(None)(None)
    with pytest.raises(ValueError, match="complex64"):
        cgmm.cgmm_masks(np.zeros((2, 5, 17), np.complex64))
    with pytest.raises(ValueError, match="empty"):
        cgmm.cgmm_masks([])
