"""The resampler's host side (no GPU): the float64 restatement of Kaldi's LinearResample reproduces the tables worked out for
DESIGN.md 7.7; the library's plan agrees with it tap for tap; WaveAugment's draws and configuration checks."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402

from pykaldi2_amd import _lib, augment  # noqa: E402

TABLE = {   # fi, fo: (iu, ou, taps range, first[0], phase-sum range, max sum |w|)
    (14400, 16000): (9, 10, (12, 13), -6, (1.00004, 1.00088), 1.869),
    (17600, 16000): (11, 10, (13, 14), -6, (1.00032, 1.00062), 1.742),
    (16000, 8000): (2, 1, (25, 25), -12, (1.00046, 1.00046), 1.455),
    (8000, 16000): (1, 2, (12, 13), -6, (1.00004, 1.00088), 1.869),
    (48000, 16000): (3, 1, (37, 37), -18, (1.00047, 1.00047), 1.521),
    (15217, 16000): (15217, 16000, (12, 13), -6, (1.00004, 1.00088), 1.869),
}


@pytest.mark.parametrize("ratio", RR.RATIOS)
def test_restatement_reproduces_the_tables(ratio):
    iu, ou, taps_range, first0, sums, abs_sum = TABLE[ratio]
    got_iu, got_ou, first, taps, w = RR.plan(*ratio)
    assert (got_iu, got_ou) == (iu, ou)
    assert (int(taps.min()), int(taps.max())) == taps_range and int(first[0]) == first0
    s = w.sum(axis=1)
    assert 1.0 <= s.min() and s.max() <= 1.001
    assert abs(s.min() - sums[0]) < 6e-6 and abs(s.max() - sums[1]) < 6e-6
    assert abs(np.abs(w).sum(axis=1).max() - abs_sum) < 6e-4


def test_restatement_output_lengths():
    ns = [1, 2, 9, 10, 11, 13, 14, 100]
    assert [RR.num_output(n, 9, 10) for n in ns] == [2, 3, 10, 12, 13, 15, 16, 112]
    assert [RR.num_output(n, 11, 10) for n in ns] == [1, 2, 9, 10, 10, 12, 13, 91]
    assert [len(RR.resample(np.ones(n), 14400, 16000)) for n in ns] == [2, 3, 10, 12, 13, 15, 16, 112]


def test_restatement_resamples_a_sine():
    """440 Hz, 4000 samples at 14400 Hz -> 4445 samples at 16000 Hz; away from the ends the error is the phase-sum ripple
    (8.8e-4 at most), measured 3.5e-4."""
    x = np.sin(2 * np.pi * 440.0 * np.arange(4000) / 14400.0)
    y = RR.resample(x, 14400, 16000)
    assert y.shape == (4445,)
    want = np.sin(2 * np.pi * 440.0 * np.arange(4445) / 16000.0)
    assert np.abs(y - want)[50:-50].max() < 1e-3


def test_restatement_equal_rates_is_identity():
    x = np.random.default_rng(0).standard_normal(37)
    assert np.array_equal(RR.resample(x, 16000, 16000), x)
    assert np.array_equal(RR.resample(x, 16000, 16000, gain=0.5), 0.5 * x)


@pytest.mark.parametrize("ratio", RR.RATIOS)
def test_library_plan_matches_the_restatement(ratio):
    plan = augment.ResamplePlan(*ratio)
    iu, ou, first, taps, w64 = RR.plan(*ratio)
    assert (plan.iu, plan.ou, plan.max_taps) == (iu, ou, w64.shape[1])
    assert plan.tile >= 256 and plan.tile % 256 == 0 and plan.table_bytes >= ou * (8 + 4 * plan.max_taps)
    gf, gt, gw = plan.export()
    assert np.array_equal(gf, first) and np.array_equal(gt, taps)
    want = w64.astype(np.float32)
    # both sides round a double to float32 once; the two doubles may differ in the last bit of sin / cos
    assert (np.abs(gw.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert (gw[np.arange(w64.shape[1])[None, :] >= taps[:, None]] == 0).all()
    assert augment.ResamplePlan(*ratio) is plan                 # cached per argument tuple


def test_library_identity_plan():
    plan = augment.ResamplePlan(16000, 16000)
    first, taps, w = plan.export()
    assert (plan.iu, plan.ou, plan.max_taps) == (1, 1, 1)
    assert first.tolist() == [0] and taps.tolist() == [1] and w.tolist() == [[1.0]]
    assert plan.num_output(12345) == 12345


@pytest.mark.parametrize("ratio", [(14400, 16000), (17600, 16000), (48000, 16000), (15217, 16000)])
def test_library_num_output(ratio):
    plan = augment.ResamplePlan(*ratio)
    fi, fo = ratio
    for n in list(range(1, 201)) + [10 ** 9]:
        assert plan.num_output(n) == -(-n * fo // fi)           # ceil(n fo / fi) in integers
        assert n > 200 or plan.num_output(n) == math.ceil(n * fo / fi)
    assert _lib.lib().pk2_resample_num_output(plan.handle, -1) == -1
    assert _lib.lib().pk2_resample_num_output(None, 5) == -1


def test_library_bad_arguments_fail_loudly():
    L = _lib.lib()
    h = C.c_void_p()

    def bad(*a):
        rc = L.pk2_resample_plan_create(*a)
        assert rc < 0 and L.pk2_last_error(), a
        with pytest.raises(_lib.Pk2Error):
            _lib.check(rc)
    assert L.pk2_resample_plan_create(14400, 16000, 0.0, 6, None) < 0 and b"null" in L.pk2_last_error().lower()
    bad(0, 16000, 0.0, 6, C.byref(h))
    bad(16000, -1, 0.0, 6, C.byref(h))
    bad(14400, 16000, 0.0, 0, C.byref(h))
    bad(14400, 16000, 7200.5, 6, C.byref(h))          # above 0.5 * min(fi, fo)
    bad(14400, 16000, -1.0, 6, C.byref(h))
    assert not h.value
    assert L.pk2_resample_plan_info(None, None, None, None, None, None) < 0 and b"null" in L.pk2_last_error().lower()
    plan = augment.ResamplePlan(14400, 16000)
    assert L.pk2_resample_plan_export(plan.handle, None, None, None) < 0 and b"null" in L.pk2_last_error().lower()
    assert L.pk2_resample_last_path(None) < 0 and b"null" in L.pk2_last_error().lower()
    assert L.pk2_resample_batch(None, 1, None) < 0
    jobs = (_lib.ResampleJob * 1)()
    assert L.pk2_resample_batch(jobs, _lib.RESAMPLE_MAX_JOBS + 1, None) < 0
    assert L.pk2_resample_batch(jobs, 1, None) < 0 and b"job 0" in L.pk2_last_error()      # null plan and pointers
    with pytest.raises(_lib.Pk2Error):
        augment.ResamplePlan(16000, 16000 // 64)        # one tile would read more input than the kernel stages
    assert L.pk2_resample_plan_destroy(None) == 0
    # a custom cutoff at the limit is accepted and owned by the caller
    assert L.pk2_resample_plan_create(16000, 8000, 4000.0, 2, C.byref(h)) == 0 and h.value
    assert L.pk2_resample_plan_destroy(h) == 0


def test_wave_augment_from_config():
    assert augment.WaveAugment.from_config({}, 0) is None
    assert augment.WaveAugment.from_config(dict(data_config=dict(simulation_prob=0)), 0) is None
    a = augment.WaveAugment.from_config(dict(data_config=dict(speed_perturb=[0.9, 1.0, 1.1])), 3)
    assert a.speed_factors == [0.9, 1.0, 1.1] and a.volume_range is None and a.seed == 3 and a.changes_length()
    assert a.ratios([0.9, 1.0, 1.1]) == [(14400, 16000), (16000, 16000), (17600, 16000)]
    b = augment.WaveAugment.from_config(dict(data_config=dict(volume_perturb=[0.125, 2.0])), 0)
    assert b.speed_factors is None and b.volume_range == (0.125, 2.0) and not b.changes_length()
    assert not augment.WaveAugment([1.0], [1.0, 1.0]).changes_length()


def test_wave_augment_draws_depend_on_seed_rank_epoch_only():
    a = augment.WaveAugment([0.9, 1.0, 1.1], [0.125, 2.0], seed=5)
    np.random.seed(123)
    before = np.random.get_state()
    f1, g1 = a.draw(a.generator(2, 7), 64)
    np.random.seed(99)          # numpy's global stream plays no part
    np.random.random(10)
    np.random.seed(123)
    f2, g2 = augment.WaveAugment([0.9, 1.0, 1.1], [0.125, 2.0], seed=5).draw(a.generator(2, 7), 64)
    after = np.random.get_state()
    assert f1 == f2 and g1 == g2
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert set(f1) == {0.9, 1.0, 1.1} and all(0.125 <= g <= 2.0 for g in g1) and len(set(g1)) == 64
    want = np.random.default_rng([5, 2, 7, 104729])
    assert f1 == [[0.9, 1.0, 1.1][int(i)] for i in want.integers(3, size=64)]
    for other in ((5, 2, 8), (5, 3, 7), (6, 2, 7)):
        o = augment.WaveAugment([0.9, 1.0, 1.1], [0.125, 2.0], seed=other[0])
        assert o.draw(o.generator(other[1], other[2]), 64) != (f1, g1)
    f, g = augment.WaveAugment([1.0], [1.0, 1.0]).draw(a.generator(0, 0), 4)
    assert f == [1.0] * 4 and g == [1.0] * 4


@pytest.mark.parametrize("dc", [dict(speed_perturb=[]), dict(speed_perturb=[0.4]), dict(speed_perturb=[1.0, 2.5]),
                                dict(speed_perturb=0.9), dict(volume_perturb=[2.0, 0.125]), dict(volume_perturb=[1.0]),
                                dict(speed_perturb=[float("nan")])])
def test_wave_augment_rejects_bad_values(dc):
    with pytest.raises(ValueError):
        augment.WaveAugment.from_config(dict(data_config=dc), 0)


def test_label_trainers_refuse_speed_perturb(capsys):
    augment.refuse_speed_perturb(dict(data_config=dict(volume_perturb=[0.5, 2.0])), "train_ce.py")
    augment.refuse_speed_perturb(dict(data_config=dict(speed_perturb=[1.0])), "train_ce.py")
    with pytest.raises(SystemExit) as e:
        augment.refuse_speed_perturb(dict(data_config=dict(speed_perturb=[0.9, 1.0])), "train_ce.py")
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "speed_perturb" in err and "train_ce.py" in err and err.count("\n") == 1
