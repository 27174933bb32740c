"""pk2_resample_batch (csrc/resample.hip) on the GPU against the float64 restatement of Kaldi's LinearResample
(tests/resample_ref.py) evaluated with the plan's exported float32 weights.

Tolerance: |y[k] - y64[k]| <= (taps + 2) 2^-24 |gain| B[k], B[k] = sum_j |w_j x_j| -- the bound of a float32 dot product of
`taps` terms plus the rounding of the gain; no measured constant.  Impulses pin every index exactly: the response to a unit
impulse is the exported weight itself (==)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402

from pykaldi2_amd import augment  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _tables(plan):
    first, taps, w = plan.export()
    return plan.iu, plan.ou, first, taps, w


def _n_in_for(plan, n_out):
    """The shortest input with at least n_out outputs."""
    fi, fo = plan.rate_in, plan.rate_out
    n = max(1, n_out * fi // fo - 2)
    while plan.num_output(n) < n_out:
        n += 1
    return n


def _run(plan, x, n_out=None, gain=1.0):
    """One job through the library; n_out defaults to the full length."""
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.empty(plan.num_output(len(x)) if n_out is None else n_out, dtype=torch.float32, device="cuda")
    augment._launch([(plan, xd, out, float(gain))], xd.device)
    return out.cpu().numpy()


def _check_bound(plan, x, got, gain=1.0):
    iu, ou, first, taps, w = _tables(plan)
    want, B = RR.apply(x, iu, ou, first, taps, w, len(got), gain)
    err = np.abs(got.astype(np.float64) - want)
    bound = (taps[np.arange(len(got)) % ou] + 2) * U * abs(gain) * B
    worst = float((err - bound).max())
    print("%d -> %d n_in %d n_out %d: max err %.3e, max err / bound %.3f" % (plan.rate_in, plan.rate_out, len(x), len(got), err.max(),
                                                                               float((err / np.maximum(bound, 1e-300)).max())))
    assert worst <= 0.0, (plan.rate_in, plan.rate_out, len(x), int(np.argmax(err - bound)), worst)


@pytest.mark.parametrize("ratio", RR.RATIOS)
def test_within_the_dot_product_bound(ratio):
    plan = augment.ResamplePlan(*ratio)
    rng = np.random.default_rng(ratio[0])
    tile = plan.tile
    for n_in in (1, 2, 5, 13, 100):
        x = rng.standard_normal(n_in).astype(np.float32)
        got = _run(plan, x)
        assert got.shape == (RR.num_output(n_in, *ratio),)
        _check_bound(plan, x, got)
    for n_out in (tile - 1, tile, tile + 1, 3 * tile + 7):
        n_in = _n_in_for(plan, n_out)
        x = rng.standard_normal(n_in).astype(np.float32)
        # (n_out itself where a length has it; an up-sampling ratio that skips it converts its first n_out outputs)
        got = _run(plan, x, n_out)
        _check_bound(plan, x, got)
        full = augment.resample(torch.from_numpy(x).cuda(), *ratio).cpu().numpy()
        assert full.shape == (plan.num_output(n_in),) and np.array_equal(full[:n_out], got)
        _check_bound(plan, x, full)


@pytest.mark.parametrize("ratio", RR.RATIOS)
def test_impulse_response_is_the_exported_weight(ratio):
    plan = augment.ResamplePlan(*ratio)
    iu, ou, first, taps, w = _tables(plan)
    tile = plan.tile
    n = _n_in_for(plan, 2 * tile + 5)
    n_out = plan.num_output(n)
    span_begin = int(first[tile % ou]) + (tile // ou) * iu          # the first input the second tile stages
    assert 1 <= span_begin < n - 2
    k = np.arange(n_out, dtype=np.int64)
    u, p = k // ou, k % ou
    for q in (0, 1, n - 2, n - 1, span_begin, span_begin - 1):
        x = np.zeros(n, np.float32)
        x[q] = 1.0
        j = q - first[p] - u * iu
        ok = (j >= 0) & (j < taps[p])
        want = np.where(ok, w[p, np.clip(j, 0, w.shape[1] - 1)], np.float32(0))
        got = _run(plan, x)
        assert ok.any() and (got == want).all(), (ratio, q, np.flatnonzero(got != want)[:5])


def _ragged_case():
    rng = np.random.default_rng(11)
    ratios = [(14400, 16000), (16000, 16000), (17600, 16000), (48000, 16000), (8000, 16000)]
    lens = [3001, 777, 1, 5000, 1300]
    return ratios, lens, [rng.standard_normal(n).astype(np.float32) for n in lens]


def _run_ragged(ratios, xs, gains, pad=64, sentinel=-777.0):
    """Inputs are views into one NaN buffer (pad NaNs around every row), outputs views into a buffer of sentinels."""
    plans = [augment.ResamplePlan(*r) for r in ratios]
    n_outs = [p.num_output(len(x)) for p, x in zip(plans, xs)]
    inbuf = torch.full((sum(len(x) for x in xs) + pad * (len(xs) + 1),), float("nan"), dtype=torch.float32, device="cuda")
    outbuf = torch.full((sum(n_outs) + pad * (len(xs) + 1),), sentinel, dtype=torch.float32, device="cuda")
    jobs, a, b, views = [], pad, pad, []
    for p, x, m, g in zip(plans, xs, n_outs, gains):
        inbuf[a:a + len(x)] = torch.from_numpy(x).cuda()
        jobs.append((p, inbuf[a:a + len(x)], outbuf[b:b + m], g))
        views.append((b, m))
        a, b = a + len(x) + pad, b + m + pad
    augment._launch(jobs, inbuf.device)
    out = outbuf.cpu().numpy()
    keep = np.ones(out.shape[0], bool)
    for b, m in views:
        keep[b:b + m] = False
    return [out[b:b + m] for b, m in views], out[keep]


def test_poisoned_surroundings_independence_and_reproducibility():
    ratios, lens, xs = _ragged_case()
    gains = [1.0, 1.0, 0.5, 1.0, 2.0]
    rows, outside = _run_ragged(ratios, xs, gains)
    assert augment.last_path() == augment.PATH_LDS
    assert (outside == -777.0).all()                                  # nothing written outside [0, n_out) of any row
    for r, y in zip(ratios, rows):
        assert np.isfinite(y).all(), r                                 # no NaN from outside [0, n_in) of any row
    assert np.array_equal(rows[1], xs[1])                              # rate_in == rate_out: the copy
    assert rows[2].shape == (1,)
    again, _ = _run_ragged(ratios, xs, gains)
    for r, x, g, y, y2 in zip(ratios, xs, gains, rows, again):
        alone = augment.resample(torch.from_numpy(x).cuda(), r[0], r[1], gain=g).cpu().numpy()
        assert np.array_equal(y, alone) and np.array_equal(y, y2), r
        _check_bound(augment.ResamplePlan(*r), x, y, g)


def test_resample_ragged_layout_and_rows():
    ratios, lens, xs = _ragged_case()
    wav = torch.from_numpy(np.concatenate(xs)).cuda()
    out, new_lens = augment.resample_ragged(wav, lens, ratios)
    assert new_lens == [RR.num_output(n, *r) for n, r in zip(lens, ratios)] and out.shape == (sum(new_lens),)
    off = 0
    for r, x, m in zip(ratios, xs, new_lens):
        assert np.array_equal(out[off:off + m].cpu().numpy(), augment.resample(torch.from_numpy(x).cuda(), *r).cpu().numpy())
        off += m
    same, same_lens = augment.resample_ragged(wav, lens, [(16000, 16000)] * 5)
    assert same is wav and same_lens == lens
    sp, sp_lens = augment.speed_perturb(wav, lens, [0.9, 1.0, 1.1, 1.0, 0.9])
    assert sp_lens == [RR.num_output(n, *r) for n, r in zip(lens, [(14400, 16000), (16000, 16000), (17600, 16000),
                                                                    (16000, 16000), (14400, 16000)])]
    two = augment.resample(torch.from_numpy(np.stack([xs[0], xs[0][::-1].copy()])).cuda(), 14400, 16000)
    assert two.shape == (2, new_lens[0]) and np.array_equal(two[0].cpu().numpy(), out[:new_lens[0]].cpu().numpy())
    # more jobs than one launch takes: split over launches, same rows
    many = 70
    wav2 = torch.from_numpy(np.concatenate([xs[4]] * many)).cuda()
    out2, lens2 = augment.resample_ragged(wav2, [lens[4]] * many, [ratios[4]] * many)
    assert lens2 == [new_lens[4]] * many
    assert (out2.view(many, -1) == out2[:new_lens[4]]).all()


def test_gain_is_one_multiplication_of_the_result():
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(2500).astype(np.float32)).cuda()
    for ratio in ((14400, 16000), (16000, 16000)):
        plain = augment.resample(x, *ratio)
        assert torch.equal(augment.resample(x, *ratio, gain=0.37), plain * 0.37)


def test_weight_paths(monkeypatch):
    rng = np.random.default_rng(5)
    coprime = augment.ResamplePlan(15217, 16000)
    x = rng.standard_normal(160000).astype(np.float32)
    got = _run(coprime, x)
    assert augment.last_path() == augment.PATH_MEM and got.shape == (RR.num_output(160000, 15217, 16000),)
    _check_bound(coprime, x, got)
    plan = augment.ResamplePlan(14400, 16000)
    x = rng.standard_normal(20000).astype(np.float32)
    lds = _run(plan, x)
    assert augment.last_path() == augment.PATH_LDS
    _check_bound(plan, x, lds)
    monkeypatch.setenv("PK2_RESAMPLE_WEIGHTS", "mem")            # the same tables read from memory: the same bits
    mem = _run(plan, x)
    assert augment.last_path() == augment.PATH_MEM and np.array_equal(mem, lds)
