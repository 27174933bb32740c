"""pk2_spec_augment / augment.spec_augment against the numpy restatement tests/specaug_ref.py: masks bit for bit (in place
and out of place), the warp within the bound of its three float32 roundings, no reads across utterances, the utterance
search over many short utterances, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import specaug_ref as SR  # noqa: E402

from pykaldi2_amd import _lib, augment  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC01234        # a quiet NaN with a payload
DENORMAL_BITS = 0x00000123
NEG_ZERO_BITS = 0x80000000


def _features(frames, seed=0):
    """Distinct bit patterns: float32 normals from a seeded generator, made unique by their index in the low mantissa."""
    rows = int(sum(frames))
    x = np.random.default_rng(seed).standard_normal((rows, 80)).astype(np.float32)
    bits = x.view(np.uint32)
    bits &= np.uint32(0xFFFE0000)
    bits |= np.arange(rows * 80, dtype=np.uint32).reshape(rows, 80) & np.uint32(0x1FFFF)
    assert len(np.unique(bits)) == bits.size
    return x


def _row_off(frames):
    off = np.zeros(len(frames) + 1, np.int64)
    off[1:] = np.cumsum(frames)
    return torch.from_numpy(off).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(x, frames, plan, fill=0.0, out=None):
    feats = torch.from_numpy(x.copy()).cuda()
    got = augment.spec_augment(feats, _row_off(frames), frames, plan, fill, out=feats if out == "inplace" else out)
    torch.cuda.synchronize()
    return feats, got


MASK_FRAMES = [1, 7, 130]        # 138 rows: the last utterance straddles the 32-row tiles of the kernel


def _mask_case():
    x = _features(MASK_FRAMES)
    xb = x.view(np.uint32)
    plan = np.stack([
        SR.plan_row(freq=[(3, 5)], time=[(0, 0)]),                                     # T = 1: nothing in time
        SR.plan_row(freq=[(0, 1), (79, 80), (3, 5)], time=[(0, 1), (6, 7), (2, 4), (3, 5), (5, 5)]),
        SR.plan_row(freq=[(0, 1), (79, 80), (3, 5), (30, 30)],
                    time=[(0, 1), (129, 130), (10, 20), (15, 25), (40, 40)] + [(50 + 5 * k, 52 + 5 * k) for k in range(11)]),
    ])
    # special values in cells no interval covers
    xb[0, 10], xb[0, 11], xb[0, 12] = NAN_BITS, DENORMAL_BITS, NEG_ZERO_BITS           # utterance 0, frame 0
    xb[1 + 1, 6], xb[1 + 1, 7], xb[1 + 1, 40] = NAN_BITS, DENORMAL_BITS, NEG_ZERO_BITS  # utterance 1, frame 1, next to [3, 5)
    xb[8 + 33, 2], xb[8 + 33, 5], xb[8 + 33, 78] = NAN_BITS, DENORMAL_BITS, NEG_ZERO_BITS
    return x, plan


@pytest.mark.parametrize("fill", [0.0, -1.5])
def test_masks_in_place_match_the_restatement_bit_for_bit(fill):
    x, plan = _mask_case()
    want, exact, _, _ = SR.spec_augment(x, MASK_FRAMES, plan, fill)
    assert exact.all()
    for cell in ((0, 10), (2, 6), (41, 2)):
        assert want[cell] == NAN_BITS             # the special values are in unmasked cells
    feats, got = _run(x, MASK_FRAMES, plan, fill, out="inplace")
    assert got is feats
    assert (_bits(got) == want).all()
    feats, got = _run(x, MASK_FRAMES, plan, fill)            # out=None without a warp: in place too
    assert got is feats and (_bits(got) == want).all()


def test_a_full_band_and_every_slot():
    frames = [40]
    x = _features(frames, seed=1)
    plan = SR.plan_row(freq=[(0, 80)])[None, :]
    _, got = _run(x, frames, plan, -1.5)
    assert (_bits(got) == np.float32(-1.5).view(np.uint32)).all()
    plan = SR.plan_row(freq=[(8, 12), (12, 13), (1, 3), (77, 79)], time=[(2 * k, 2 * k + 1) for k in range(16)])[None, :]
    want, _, _, _ = SR.spec_augment(x, frames, plan, 0.0)
    _, got = _run(x, frames, plan, 0.0)
    assert (_bits(got) == want).all()
    assert (_bits(got)[0:32:2] == 0).all() and (_bits(got)[1:32:2, 20] != 0).all()


def test_out_of_place_without_a_warp_leaves_the_input_alone():
    x, plan = _mask_case()
    want, _, _, _ = SR.spec_augment(x, MASK_FRAMES, plan, -1.5)
    out = torch.full((sum(MASK_FRAMES), 80), 7.0, device="cuda")
    feats, got = _run(x, MASK_FRAMES, plan, -1.5, out=out)
    assert got is out
    assert (_bits(got) == want).all()
    assert (_bits(feats) == x.view(np.uint32)).all()


def _check_warp(x, frames, plan, got, fill=0.0):
    want, exact, ref64, bound = SR.spec_augment(x, frames, plan, fill)
    gb = _bits(got)
    assert (gb[exact] == want[exact]).all()
    g = got.cpu().numpy().astype(np.float64)
    err = np.abs(g - ref64)[~exact]
    # one rounded quotient, one rounded difference, one fused multiply-add
    assert (err <= 4.0 * 2.0 ** -24 * bound[~exact]).all(), float((err / bound[~exact]).max() * 2.0 ** 24)
    return exact


def test_warp_matches_the_float64_restatement():
    frames = [5, 5, 5, 130, 130, 130, 130]
    plan = np.stack([SR.plan_row(c=2, d=1), SR.plan_row(c=2, d=2), SR.plan_row(c=2, d=3), SR.plan_row(c=41, d=1),
                     SR.plan_row(c=41, d=81), SR.plan_row(c=87, d=47), SR.plan_row(c=87, d=127)])
    x = _features(frames, seed=2)
    feats, got = _run(x, frames, plan)
    assert got is not feats                                   # out=None with a warp: a new tensor
    assert (_bits(feats) == x.view(np.uint32)).all()
    exact = _check_warp(x, frames, plan, got)
    assert (~exact).any(axis=1).sum() > 300                   # most frames of the long utterances are interpolated
    off = np.concatenate([[0], np.cumsum(frames)])
    gb, xb = _bits(got), x.view(np.uint32)
    for n in range(len(frames)):                              # first and last frame map to themselves
        assert (gb[off[n]] == xb[off[n]]).all() and (gb[off[n + 1] - 1] == xb[off[n + 1] - 1]).all()
    assert (gb[5:10] == xb[5:10]).all()                       # c == d: the identity
    # the centre moves to d: out[d] = in[c]
    for n, (c, d) in enumerate([(2, 1), (2, 2), (2, 3), (41, 1), (41, 81), (87, 47), (87, 127)]):
        assert (gb[off[n] + d] == xb[off[n] + c]).all()


def test_no_reads_across_utterances():
    frames = [9, 33, 9]
    x = _features(frames, seed=3)
    x[:9], x[42:] = np.nan, np.nan
    plan = np.stack([SR.plan_row(), SR.plan_row(c=16, d=30), SR.plan_row()])
    _, got = _run(x, frames, plan)
    g = got.cpu().numpy()
    assert np.isnan(g[:9]).all() and np.isnan(g[42:]).all() and not np.isnan(g[9:42]).any()
    _check_warp(x, frames, plan, got)


def test_masks_land_at_output_coordinates_after_the_warp():
    frames = [3, 130]
    x = _features(frames, seed=4)
    plan = np.stack([SR.plan_row(time=[(1, 2)]),
                     SR.plan_row(c=41, d=81, freq=[(3, 5), (79, 80)], time=[(81, 83), (0, 1), (100, 110)])])
    _, got = _run(x, frames, plan, -1.5)
    exact = _check_warp(x, frames, plan, got, -1.5)
    assert not exact.all()
    g = got.cpu().numpy()
    masked_rows = [3 + t for t in [0, 81, 82] + list(range(100, 110))] + [1]
    assert (g[masked_rows] == -1.5).all()
    assert (g[[0, 2]] != -1.5).all()                          # the short utterance has no frequency mask
    others = np.setdiff1d(np.arange(3, 133), masked_rows)
    assert (g[others][:, [3, 4, 79]] == -1.5).all() and (g[others][:, [2, 5, 78]] != -1.5).all()


def test_many_short_utterances():
    rng = np.random.default_rng(5)
    frames = [int(t) for t in rng.integers(1, 4, size=300)]
    assert set(frames) == {1, 2, 3}
    plan = np.stack([SR.plan_row(freq=[(n % 80, n % 80 + 1)], time=[(a, a + 1)])
                     for n, a in enumerate(int(rng.integers(0, t)) for t in frames)])
    x = _features(frames, seed=6)
    want, exact, _, _ = SR.spec_augment(x, frames, plan, 0.0)
    assert exact.all()
    _, got = _run(x, frames, plan, 0.0)
    assert (_bits(got) == want).all()
    _, got = _run(x, frames, plan, 0.0, out=torch.empty(sum(frames), 80, device="cuda"))
    assert (_bits(got) == want).all()


def test_refusals():
    frames = [7]
    x = _features(frames)
    feats = torch.from_numpy(x).cuda()
    off = _row_off(frames)
    warp = SR.plan_row(c=2, d=4)[None, :]
    with pytest.raises(ValueError, match="in place"):
        augment.spec_augment(feats, off, frames, warp, out=feats)
    plan_dev = torch.from_numpy(warp).cuda()
    call = _lib.lib().pk2_spec_augment
    stream = _lib.stream_ptr(feats.device)
    rc = call(_lib.ptr(feats), _lib.ptr(feats), _lib.ptr(off), 1, 7, _lib.ptr(plan_dev), 1, 0.0, stream)
    assert rc != 0 and b"in place" in _lib.lib().pk2_last_error()
    out = torch.empty_like(feats)
    for args in ((None, _lib.ptr(out), _lib.ptr(off), 1, 7, _lib.ptr(plan_dev)),
                 (_lib.ptr(feats), None, _lib.ptr(off), 1, 7, _lib.ptr(plan_dev)),
                 (_lib.ptr(feats), _lib.ptr(out), None, 1, 7, _lib.ptr(plan_dev)),
                 (_lib.ptr(feats), _lib.ptr(out), _lib.ptr(off), 1, 7, None)):
        rc = call(*args, 0, 0.0, stream)
        assert rc < 0 and b"null" in _lib.lib().pk2_last_error().lower()
    assert call(_lib.ptr(feats), _lib.ptr(out), _lib.ptr(off), 0, 7, _lib.ptr(plan_dev), 0, 0.0, stream) < 0
    assert call(_lib.ptr(feats), _lib.ptr(out), _lib.ptr(off), 1, 0, _lib.ptr(plan_dev), 0, 0.0, stream) < 0
    with pytest.raises(_lib.Pk2Error):
        _lib.check(call(_lib.ptr(feats), _lib.ptr(out), _lib.ptr(off), 1, 0, _lib.ptr(plan_dev), 0, 0.0, stream))
    torch.cuda.synchronize()
    assert (_bits(feats) == x.view(np.uint32)).all()          # no refused call wrote anything
    with pytest.raises(ValueError, match="feats"):
        augment.spec_augment(feats[:6], off, frames, SR.plan_row()[None, :])


def test_call_is_deterministic_for_equal_rank_and_epoch():
    frames = [130, 61, 5]
    x = _features(frames, seed=7)
    aug = augment.SpecAugment(time_warp=2, fill=-1.5, seed=9)
    off = _row_off(frames)
    a = aug(torch.from_numpy(x.copy()).cuda(), off, frames, aug.generator(1, 3))
    b = aug(torch.from_numpy(x.copy()).cuda(), off, frames, aug.generator(1, 3))
    c = aug(torch.from_numpy(x.copy()).cuda(), off, frames, aug.generator(1, 4))
    assert (_bits(a) == _bits(b)).all() and (_bits(a) != _bits(c)).any()
    assert (a == -1.5).any() and (_bits(a) != x.view(np.uint32)).any()
    # the callable of an epoch draws on: two calls of one epoch differ, the same calls of an equal epoch agree
    e1, e2 = aug.epoch(0, 0), aug.epoch(0, 0)
    first = [e(torch.from_numpy(x.copy()).cuda(), off, frames) for e in (e1, e2)]
    second = [e(torch.from_numpy(x.copy()).cuda(), off, frames) for e in (e1, e2)]
    assert (_bits(first[0]) == _bits(first[1])).all() and (_bits(second[0]) == _bits(second[1])).all()
    assert (_bits(first[0]) != _bits(second[0])).any()
