"""SpecAugment's host side (no GPU): configuration parsing and checks, the bounds and the reproducibility of the draws, the
start-up refusal of a time warp, and the plan validation of augment.spec_augment, which runs before anything needs a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import specaug_ref as SR  # noqa: E402

from pykaldi2_amd import _lib, augment  # noqa: E402


def _cfg(value):
    return {"data_config": {"spec_augment": value}}


def test_constants_match_the_restatement():
    assert (_lib.SPEC_MAX_FREQ_MASKS, _lib.SPEC_MAX_TIME_MASKS, _lib.SPEC_PLAN_STRIDE) == (SR.MAX_FREQ, SR.MAX_TIME, SR.STRIDE) \
        == (4, 16, 42)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pk2hip.h")).read()
    assert "#define PK2_SPEC_MAX_FREQ_MASKS 4\n" in hdr and "#define PK2_SPEC_MAX_TIME_MASKS 16\n" in hdr


def test_from_config_defaults_mapping_and_absence():
    a = augment.SpecAugment.from_config(_cfg(True), seed=5)
    assert (a.freq_masks, a.freq_width, a.time_masks, a.time_width, a.time_ratio, a.time_warp, a.fill, a.seed) == \
        (2, 27, 2, 40, 0.2, 0, 0.0, 5)
    b = augment.SpecAugment.from_config(_cfg({"time_warp": 5, "freq_masks": 1, "fill": -1.5, "time_ratio": 1}), seed=0)
    assert (b.freq_masks, b.freq_width, b.time_masks, b.time_width, b.time_ratio, b.time_warp, b.fill) == \
        (1, 27, 2, 40, 1.0, 5, -1.5)
    assert augment.SpecAugment.from_config({"data_config": {}}) is None
    assert augment.SpecAugment.from_config({}) is None
    assert augment.SpecAugment.from_config(_cfg(False)) is None
    assert augment.SpecAugment.from_config(_cfg(None)) is None
    with pytest.raises(KeyError, match="time_wrap"):
        augment.SpecAugment.from_config(_cfg({"time_wrap": 5}))


@pytest.mark.parametrize("key,value", [("freq_masks", 5), ("freq_masks", -1), ("freq_masks", 1.5), ("time_masks", 17),
                                       ("time_masks", -1), ("freq_width", 81), ("freq_width", -1), ("time_width", -1),
                                       ("time_ratio", 1.01), ("time_ratio", -0.1), ("time_ratio", float("nan")),
                                       ("time_warp", -1), ("time_warp", 2.5), ("fill", float("inf")), ("fill", float("nan")),
                                       ("fill", "mean")])
def test_bad_values_name_their_key(key, value):
    with pytest.raises(ValueError, match=key):
        augment.SpecAugment(**{key: value})
    with pytest.raises(ValueError, match=key):
        augment.SpecAugment.from_config(_cfg({key: value}))


def test_limits_are_accepted():
    a = augment.SpecAugment(freq_masks=4, freq_width=80, time_masks=16, time_width=0, time_ratio=1.0, time_warp=0, fill=-3)
    plan = a.draw(a.generator(), [7])
    assert plan.shape == (1, 42) and (plan[0, SR.TIME0:] .reshape(-1, 2)[:, 0] == plan[0, SR.TIME0:].reshape(-1, 2)[:, 1]).all()


@pytest.mark.parametrize("T", [1, 2, 4, 5, 130])
def test_draws_stay_inside_their_bounds(T):
    W = 1 if T <= 5 else 40
    a = augment.SpecAugment(freq_masks=4, freq_width=27, time_masks=16, time_width=40, time_ratio=0.2, time_warp=W)
    plan = a.draw(a.generator(0, 0), [T] * 1000)
    assert plan.dtype == np.int32 and plan.shape == (1000, _lib.SPEC_PLAN_STRIDE)
    c, d = plan[:, 0], plan[:, 1]
    if T >= 2 * W + 3:
        assert (c >= W + 1).all() and (c <= T - W - 2).all() and (np.abs(d - c) <= W).all()
        assert (d >= 1).all() and (d <= T - 2).all()
        assert len(set((d - c).tolist())) == 2 * W + 1          # every shift in [-W, W] is drawn
        if T == 5:
            assert (c == 2).all()
        else:
            assert c.min() == W + 1 and c.max() == T - W - 2
    else:
        assert (c == 0).all() and (d == 0).all()                # T = 4 with W = 1 does not warp
    fa, fb = plan[:, SR.FREQ0:SR.TIME0:2], plan[:, SR.FREQ0 + 1:SR.TIME0:2]
    assert (fa >= 0).all() and (fb <= 80).all() and (fb - fa >= 0).all() and (fb - fa <= 27).all()
    assert (fb - fa).max() == 27 and (fb - fa).min() == 0 and fa.min() == 0 and fb.max() == 80
    ta, tb = plan[:, SR.TIME0::2], plan[:, SR.TIME0 + 1::2]
    widest = min(40, int(np.floor(0.2 * T)))
    assert (ta >= 0).all() and (tb <= T).all() and (tb - ta >= 0).all() and (tb - ta <= widest).all()
    assert (tb - ta).max() == widest
    if T == 1:
        assert (tb == ta).all()                                  # time width 0
    assert augment._check_plan(plan, [T] * 1000) == (T >= 2 * W + 3)


def test_unused_slots_are_empty():
    a = augment.SpecAugment(freq_masks=1, time_masks=3)
    plan = a.draw(a.generator(), [130, 60])
    assert (plan[:, SR.FREQ0 + 2:SR.TIME0] == 0).all() and (plan[:, SR.TIME0 + 6:] == 0).all() and (plan[:, :2] == 0).all()


def test_draws_depend_on_seed_rank_and_epoch_only():
    frames = [130, 61, 200, 5]
    a = augment.SpecAugment(time_warp=2, seed=3)
    ref = a.draw(a.generator(1, 2), frames)
    assert (augment.SpecAugment(time_warp=2, seed=3).draw(a.generator(1, 2), frames) == ref).all()
    for other in (a.generator(0, 2), a.generator(1, 3), augment.SpecAugment(time_warp=2, seed=4).generator(1, 2)):
        assert (a.draw(other, frames) != ref).any()
    # a stream of its own: not WaveAugment's
    w = augment.WaveAugment([0.9, 1.0, 1.1], None, seed=3)
    assert a.generator(1, 2).integers(1 << 30) != w.generator(1, 2).integers(1 << 30)


def test_draws_leave_the_global_stream_alone():
    np.random.seed(11)
    before = np.random.get_state()
    a = augment.SpecAugment(time_warp=5)
    a.draw(a.generator(0, 0), [130, 7, 1])
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]


def test_refuse_time_warp(capsys):
    augment.refuse_time_warp({}, "train_ce.py")
    augment.refuse_time_warp(_cfg(True), "train_ce.py")
    augment.refuse_time_warp(_cfg({"time_warp": 0}), "train_ce.py")
    assert capsys.readouterr().err == ""
    with pytest.raises(SystemExit) as e:
        augment.refuse_time_warp(_cfg({"time_warp": 5}), "train_ce.py")
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.endswith("\n") and "time_warp" in err and "train_ce.py" in err


@pytest.mark.parametrize("what,row,frames", [
    ("time interval past T", SR.plan_row(time=[(5, 8)]), [7]),
    ("d = T - 1", SR.plan_row(c=3, d=6), [7]),
    ("c = 0", SR.plan_row(c=0, d=1), [7]),
    ("frequency interval past 80", SR.plan_row(freq=[(79, 81)]), [7]),
    ("reversed interval", SR.plan_row(time=[(4, 3)]), [7]),
    ("negative start", SR.plan_row(freq=[(-1, 3)]), [7]),
    ("warp of a one-frame utterance", SR.plan_row(c=1, d=0), [1]),
])
def test_spec_augment_validates_the_plan_before_the_gpu(what, row, frames):
    """feats and row_off are never looked at: the plan check comes first and needs no GPU."""
    with pytest.raises(ValueError, match="utterance 0"):
        augment.spec_augment(None, None, frames, row[None, :].copy())


def test_spec_augment_rejects_a_misshapen_plan():
    for plan in (np.zeros((2, 42), np.int32), np.zeros((1, 41), np.int32), np.zeros((1, 42), np.int64), [[0] * 42]):
        with pytest.raises(ValueError, match="plan"):
            augment.spec_augment(None, None, [7], plan)
    with pytest.raises(ValueError, match="fill"):
        augment.spec_augment(None, None, [7], np.zeros((1, 42), np.int32), fill=float("nan"))
