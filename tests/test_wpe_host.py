"""WPE without a GPU: properties of the float64 restatement (tests/wpe_ref.py), the conditions the GPU tests rely on, the
data_config key `wpe`, and the argument checks of the ABI entries, which run before the device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wpe_ref as R  # noqa: E402

from pykaldi2_amd import _lib, dereverb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_the_restatement_and_the_header():
    assert dereverb.FRAMES_PER_PART == _lib.WPE_FRAMES_PER_PART == R.P == 1024
    assert (dereverb.MAX_CHANNELS, dereverb.MAX_ORDER, dereverb.MAX_DELAY, dereverb.MAX_ITERS) == (8, 80, 8, 8)
    hdr = open(os.path.join(ROOT, "include", "pk2hip.h")).read()
    for line in ("#define PK2_WPE_MAX_CHANNELS 8\n", "#define PK2_WPE_MAX_ORDER 80\n", "#define PK2_WPE_MAX_DELAY 8\n",
                 "#define PK2_WPE_MAX_ITERS 8\n", "#define PK2_WPE_MAX_UTTS 32\n", "#define PK2_WPE_FRAMES_PER_PART 1024\n"):
        assert line in hdr


# ---------------------------------------------------------------------------------------------------------------------
# properties of the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,taps,delay", [(1, 4, 1), (3, 3, 2), (2, 5, 3)])
def test_one_unweighted_iteration_is_least_squares(Cn, taps, delay):
    """lambda = 1 and diag_load = 0: G minimises ||Y - y~ conj(G)||, so X is the residual of numpy's lstsq"""
    r = np.random.RandomState(Cn)
    N, F = 60, 5
    Y = r.standard_normal((Cn, N, F)) + 1j * r.standard_normal((Cn, N, F))
    X, bad = R.wpe(Y, taps, delay, 1, 0.0, weight=np.ones((N, F)))
    assert not bad
    past = R.stack_past(Y, taps, delay)
    for f in range(F):
        target = Y[:, :, f].T                                       # (N, C)
        coef = np.linalg.lstsq(past[f], target, rcond=None)[0]
        want = (target - past[f] @ coef).T
        assert np.abs(X[:, :, f] - want).max() <= 1e-9 * np.abs(Y).max()


def test_an_exact_ar_process_is_whitened():
    """Y(t) = a Y(t - delay) + e(t) per bin, diag_load = 0: the prediction error for t >= delay is e"""
    r = np.random.RandomState(5)
    N, F, delay = 400, 4, 2
    e = r.standard_normal((1, N, F)) + 1j * r.standard_normal((1, N, F))
    a = 0.6 * np.exp(2j * np.pi * r.rand(F))
    Y = e.copy()
    for t in range(delay, N):
        Y[0, t] += a * Y[0, t - delay]
    # a continuing innovation: the estimate is a's up to the chance correlation of e with the past (1 / sqrt(N)) ...
    G, bad = R.solve(*R.correlations(Y, np.ones((N, F)), 1, delay), 0.0)
    assert not bad.any() and np.abs(np.conj(G[:, 0, 0]) - a).max() < 0.2
    # ... and with the exact coefficient the filter returns e
    exact = R.apply(Y, np.conj(a)[:, None, None], delay)
    assert np.abs(exact[0, delay:] - e[0, delay:]).max() <= 1e-6 * np.abs(e).max()
    # an innovation that stops after the first frames leaves nothing to chance: the estimate itself recovers e
    e2 = np.zeros_like(e)
    e2[0, :delay] = e[0, :delay]
    Y2 = e2.copy()
    for t in range(delay, N):
        Y2[0, t] += a * Y2[0, t - delay]
    X2, bad = R.wpe(Y2, 1, delay, 1, 0.0, weight=np.ones((N, F)))
    assert not bad and np.abs(X2[0, delay:] - e2[0, delay:]).max() <= 1e-6 * np.abs(e2).max()


@pytest.mark.parametrize("N", [1, 2, 3])
def test_no_past_and_silence_come_back_unchanged(N):
    r = np.random.RandomState(N)
    Y = (r.standard_normal((2, N, 5)) + 1j * r.standard_normal((2, N, 5))).astype(np.complex64)
    for dtype in (np.float64, np.float32):
        X, bad = R.wpe(Y, 4, 3, 3, 1e-3, dtype)
        assert not bad and np.array_equal(X, Y) and np.isfinite(X).all()
        Z, bad = R.wpe(np.zeros((2, 50, 5), np.complex64), 4, 3, 3, 1e-3, dtype)
        assert not bad and not Z.any() and np.isfinite(Z).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_correlations_are_hermitian_with_a_real_diagonal(dtype):
    Y = R.case_input("c7_k5_d1_n33_f17")
    Rm, Pm = R.correlations(Y, R.power(Y, dtype), 5, 1, dtype)
    assert Rm.shape == (17, 35, 35) and Pm.shape == (17, 35, 7)
    assert np.array_equal(Rm, Rm.conj().transpose(0, 2, 1))
    diag = np.diagonal(Rm, axis1=-2, axis2=-1)
    assert not diag.imag.any() and (diag.real >= 0).all()


def test_a_non_finite_bin_passes_through():
    Y = R.case_input("c3_k2_d1_n97_f33_zero").copy()
    Y[1, 50, 4] = np.nan
    X, bad = R.wpe(Y, 2, 1, 2, 1e-3)
    assert bad and np.array_equal(np.ascontiguousarray(X[:, :, 4]).view(np.uint64),
                                  np.ascontiguousarray(Y[:, :, 4].astype(np.complex128)).view(np.uint64))
    keep = np.arange(33) != 4
    clean = R.wpe(R.case_input("c3_k2_d1_n97_f33_zero"), 2, 1, 2, 1e-3)[0]
    assert np.array_equal(X[:, :, keep], clean[:, :, keep])


def test_exact_integer_inputs_are_exact_in_float32():
    Y, w = R.integer_input(3, 200, 5, 1)
    a, b = R.correlations(Y, w, 4, 2), R.correlations(Y, w, 4, 2, np.float32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.abs(a[0]).max() < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------
# the late-reverberation scene
# ---------------------------------------------------------------------------------------------------------------------
def test_the_scene_loses_its_late_reverberation():
    Y, E = R.scene(4, 600, 9, 3, seed=0)
    one = R.reduction_db(R.wpe(Y, 10, 3, 1, 1e-3)[0], Y, E)
    X, bad = R.wpe(Y, 10, 3, 3, 1e-3)
    three = R.reduction_db(X, Y, E)
    X32, bad32 = R.wpe(Y.astype(np.complex64), 10, 3, 3, 1e-3, np.float32)
    three32 = R.reduction_db(X32, Y, E)
    rel = np.abs(X32 - R.wpe(Y.astype(np.complex64), 10, 3, 3, 1e-3)[0]).max() / np.abs(X).max()
    print("reduction: %.2f dB after one iteration, %.2f dB after three, %.2f dB in float32 mode (rel err %.2e)"
          % (one, three, three32, rel))
    assert not bad and not bad32
    assert one >= 3.0 and three >= 3.0
    assert abs(three32 - three) <= 0.1 and rel < 1e-3


def test_condition_every_case_of_the_gpu_tests_stays_below_1e_3_in_float32_mode():
    """The inputs of tests/test_gpu_wpe.py are well enough conditioned for a float32 front end; its tolerances are 4 x the
    largest of these figures (cases with D >= 40 use diag_load >= 1e-3: DESIGN.md 7.10)."""
    errs = R.float32_errors()
    assert set(errs) == set(R.CASES) | {"ragged_%d" % n for n in R.RAGGED["frames"]}
    for name, e in errs.items():
        assert e["wpe"] < 1e-3 and e["corr"] < 1e-5 and e["apply"] < 1e-5 and e["power"] < 1e-6, (name, e)
    for name, (Cn, taps, _, _, _, dl, _, _) in R.CASES.items():
        assert Cn * taps < 40 or dl >= 1e-3, name
    assert max(e["power"] for e in errs.values()) <= 1.49e-7 * 1.05 and max(e["corr"] for e in errs.values()) <= 1.28e-6 * 1.05
    assert max(e["apply"] for e in errs.values()) <= 9.23e-7 * 1.05 and max(e["wpe"] for e in errs.values()) <= 2.31e-4 * 1.05


# ---------------------------------------------------------------------------------------------------------------------
# data_config `wpe`
# ---------------------------------------------------------------------------------------------------------------------
def _cfg(value, **dc):
    base = dict(use_reverb=True, simulation_prob=0.5)
    base.update(dc)
    return {"data_config": dict(base, wpe=value)}


def test_config_accepted_forms():
    assert dereverb.wpe_config(_cfg(True)) == dict(taps=10, delay=3, iterations=3, diag_load=0.001)
    assert dereverb.wpe_config(_cfg({"taps": 4, "iterations": 1})) == dict(taps=4, delay=3, iterations=1, diag_load=0.001)
    assert dereverb.wpe_config(_cfg({})) == dereverb.CONFIG_DEFAULTS
    for absent in ({}, {"data_config": {}}, _cfg(False), _cfg(None), {"data_config": {"wpe": False, "simulation_prob": 0}}):
        assert dereverb.wpe_config(absent) is None
    both = _cfg(True, online_rir=True, beamform={"n_mics": 8})
    assert dereverb.wpe_config(both)["taps"] == 10


@pytest.mark.parametrize("dc,word", [(dict(use_reverb=False), "use_reverb"), (dict(simulation_prob=0), "simulation_prob")])
def test_config_names_the_missing_key(dc, word):
    with pytest.raises(ValueError, match=word):
        dereverb.wpe_config(_cfg(True, **dc))
    cfg = _cfg(True, **dc)
    for k in dc:
        del cfg["data_config"][k]
    with pytest.raises(ValueError, match=word):
        dereverb.wpe_config(cfg)


@pytest.mark.parametrize("value,word", [({"taps": 0}, "taps"), ({"taps": 81}, "taps"), ({"taps": 2.5}, "taps"),
                                        ({"delay": 0}, "delay"), ({"delay": 9}, "delay"), ({"iterations": 0}, "iterations"),
                                        ({"iterations": 9}, "iterations"), ({"iterations": True}, "iterations"),
                                        ({"diag_load": -1}, "diag_load"), ({"diag_load": float("nan")}, "diag_load"),
                                        ({"tap": 4}, "tap"), (3, "mapping")])
def test_config_bad_values_name_their_key(value, word):
    with pytest.raises(ValueError, match=word):
        dereverb.wpe_config(_cfg(value))


def test_config_refuses_an_order_above_eighty_with_the_array():
    with pytest.raises(ValueError, match="taps"):
        dereverb.wpe_config(_cfg({"taps": 12}, online_rir=True, beamform=True))       # 7 x 12 = 84
    assert dereverb.wpe_config(_cfg({"taps": 11}, online_rir=True, beamform=True))["taps"] == 11


def test_config_start_up_exit_is_one_line():
    code = ("import sys; sys.path.insert(0, %r); from pykaldi2_amd import dereverb; "
            "dereverb.require_wpe_config({'data_config': {'wpe': True, 'simulation_prob': 1}}, 'prog')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "use_reverb" in out.stderr and "Traceback" not in out.stderr
    assert len(out.stderr.strip().splitlines()) == 1


def test_pool_with_and_without_the_key():
    from pykaldi2_amd import data
    cfg = {"synthetic": True, "data_config": dict(use_reverb=True, use_dir_noise=True, simulation_prob=1.0)}
    assert data.SimulationPool.from_config(cfg).wpe is None
    cfg["data_config"]["wpe"] = {"taps": 5}
    pool = data.SimulationPool.from_config(cfg)
    assert pool.wpe == dict(taps=5, delay=3, iterations=3, diag_load=0.001) and pool.dereverb.taps == 5
    with pytest.raises(ValueError, match="use_reverb"):
        data.SimulationPool.from_config({"synthetic": True, "data_config": dict(use_dir_noise=True, simulation_prob=1.0, wpe=True)})


# ---------------------------------------------------------------------------------------------------------------------
# the ABI refuses bad arguments before it touches the device
# ---------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.lib().pk2_last_error().lower()


def test_bad_abi_arguments_fail_loudly():
    L = _lib.lib()
    one = (C.c_void_p * 4)(8, 8, 8, 8)           # never dereferenced: every call below is refused on the host
    other = (C.c_void_p * 4)(16, 16, 16, 16)
    frames = (C.c_int32 * 1)(5)
    work = C.c_void_p(8)
    big = 1 << 30
    need = L.pk2_wpe_workspace_bytes(frames, 1, 2, 17, 4, 3)
    assert need > 5 * 2 * 17 * 8
    assert L.pk2_wpe_workspace_bytes(frames, 1, 9, 17, 4, 3) == 0 and L.pk2_wpe_workspace_bytes(frames, 1, 8, 17, 11, 3) == 0
    assert L.pk2_wpe_workspace_bytes(frames, 1, 2, 17, 4, 0) == 0 and L.pk2_wpe_workspace_bytes(frames, 1, 2, 17, 4, 9) == 0
    assert L.pk2_wpe_workspace_bytes(None, 1, 2, 17, 4, 3) == 0 and L.pk2_wpe_workspace_bytes((C.c_int32 * 1)(0), 1, 2, 17, 4, 3) == 0

    def wpe(spec=one, fr=frames, B=1, Cn=2, F=17, taps=4, delay=3, iters=3, dl=1e-3, wk=work, nbytes=big, out=other, flag=work):
        return L.pk2_wpe(spec, fr, B, Cn, F, taps, delay, iters, dl, wk, nbytes, out, flag, None)
    assert wpe(Cn=9) < 0 and b"channels" in _err()
    assert wpe(Cn=8, taps=11) < 0 and b"order" in _err()                   # C * taps = 88
    assert wpe(delay=0) < 0 and b"delay" in _err()
    assert wpe(delay=9) < 0 and b"delay" in _err()
    assert wpe(iters=0) < 0 and b"iterations" in _err()
    assert wpe(iters=9) < 0 and b"iterations" in _err()
    assert wpe(spec=None) < 0 and b"null" in _err()
    assert wpe(out=None) < 0 and b"null" in _err()
    assert wpe(spec=(C.c_void_p * 1)(None)) < 0 and b"null" in _err()
    assert wpe(fr=None) < 0 and b"frames" in _err()
    assert wpe(fr=(C.c_int32 * 1)(0)) < 0 and b"frames" in _err()
    assert wpe(wk=None) < 0 and b"null" in _err()
    assert wpe(flag=None) < 0 and b"null" in _err()
    assert wpe(nbytes=need - 1) < 0 and b"workspace" in _err()
    assert wpe(out=one) < 0 and b"its spectrum" in _err()
    assert wpe(dl=-1.0) < 0 and b"diag_load" in _err()
    assert wpe(B=0) < 0 and b"no utterance" in _err()
    assert wpe(F=0) < 0 and b"bins" in _err()
    with pytest.raises(_lib.Pk2Error):
        _lib.check(wpe(Cn=9))

    assert L.pk2_wpe_power(None, frames, 1, 2, 17, one, None) < 0 and b"null" in _err()
    assert L.pk2_wpe_power(one, frames, 1, 9, 17, one, None) < 0 and b"channels" in _err()
    assert L.pk2_wpe_power(one, frames, 1, 2, 17, None, None) < 0 and b"null" in _err()
    assert L.pk2_wpe_power(one, (C.c_int32 * 1)(-2), 1, 2, 17, one, None) < 0 and b"frames" in _err()

    def corr(spec=one, wt=one, fr=frames, Cn=2, taps=4, delay=3, wk=work, nbytes=big, Rm=work, Pm=work):
        return L.pk2_wpe_corr(spec, wt, fr, 1, Cn, 17, taps, delay, wk, nbytes, Rm, Pm, None)
    assert corr(Cn=9) < 0 and b"channels" in _err()
    assert corr(Cn=8, taps=11) < 0 and b"order" in _err()
    assert corr(delay=0) < 0 and corr(delay=9) < 0 and b"delay" in _err()
    assert corr(spec=None) < 0 and b"null" in _err()
    assert corr(wt=None) < 0 and b"null" in _err()
    assert corr(Rm=None) < 0 and b"null" in _err()
    assert corr(nbytes=need - 1) < 0 and b"workspace" in _err()

    def solve(Rm=work, Pm=work, Cn=2, taps=4, dl=1e-3, wk=work, nbytes=big, G=work, flag=work):
        return L.pk2_wpe_solve(Rm, Pm, 1, Cn, 17, taps, dl, wk, nbytes, G, flag, None)
    assert solve(Cn=9) < 0 and b"channels" in _err()
    assert solve(Cn=8, taps=11) < 0 and b"order" in _err()
    assert solve(Rm=None) < 0 and b"null" in _err()
    assert solve(flag=None) < 0 and b"null" in _err()
    assert solve(dl=float("nan")) < 0
    assert solve(nbytes=8) < 0 and b"workspace" in _err()

    def filt(spec=one, G=work, fr=frames, Cn=2, taps=4, delay=3, out=other, pw=None):
        return L.pk2_wpe_filter(spec, G, fr, 1, Cn, 17, taps, delay, out, pw, None)
    assert filt(Cn=9) < 0 and b"channels" in _err()
    assert filt(Cn=8, taps=11) < 0 and b"order" in _err()
    assert filt(delay=0) < 0 and filt(delay=9) < 0 and b"delay" in _err()
    assert filt(G=None) < 0 and b"null" in _err()
    assert filt(out=None) < 0 and b"null" in _err()
    assert filt(out=one) < 0 and b"its spectrum" in _err()
    assert filt(pw=(C.c_void_p * 1)(None)) < 0 and b"null" in _err()


def test_python_argument_errors_that_need_no_gpu():
    import torch
    for kw, word in ((dict(taps=0), "taps"), (dict(taps=81), "taps"), (dict(delay=0), "delay"), (dict(delay=9), "delay"),
                     (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(diag_load=-0.5), "diag_load")):
        with pytest.raises(ValueError, match=word):
            dereverb.Dereverberator(None, **kw)
    with pytest.raises(ValueError, match="CUDA"):
        dereverb.wpe(torch.zeros(2, 5, 17, dtype=torch.complex64))
    with pytest.raises(ValueError, match="empty"):
        dereverb.wpe([])
