"""pykaldi2_amd.beamform on the device against the float64 restatement tests/beamform_ref.py: the three kernels at the
shapes where each can go wrong, poisoned padding, exact Hermitian symmetry, batch independence and run-to-run identity bit for
bit, the 'snr' reference, the beamformer end to end, an SI-SDR gain on an anechoic scene, and SimulationPool with the
data_config key."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_ref as R  # noqa: E402

from pykaldi2_amd import _lib, beamform, simulation  # noqa: E402

pytestmark = pytest.mark.gpu

# float32 kernels against the float64 restatement.  The rule: run the restatement in float32 on the CPU
# against its float64 result over these very cases (CASES and RAGGED) and take 4 x the largest error relative to
# max|want|.  Measured with beamform_ref, never with the device:
COV_TOL = 4 * 3.91e-7        # covariance(float32): 2.78e-8 .. 3.91e-7
W_TOL = 4 * 1.78e-4          # float64 solve of the float32-summed covariances against all-float64: 1.1e-16 (C = 1) .. 1.78e-4
APPLY_TOL = 4 * 2.55e-7      # apply(float32) with the complex64 weights: 0 (C = 1) .. 2.55e-7
# end to end in float32 (STFT, covariance, apply, inverse STFT) on samples whose window sum is >= 1e-3 of its maximum
E2E_TOL = {"f257_c4": 4 * 3.37e-4, "f33_c2": 4 * 1.48e-4}
PAD = 64                     # poisoned elements behind every output
DEV = torch.device("cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _assert_hermitian(phi):
    """Phi == Phi^H exactly: the real parts bit for bit, every imaginary part the exact negative of its mirror image (which
    makes the diagonal's +0 or -0), and no NaN that would compare unequal"""
    re, im = phi.real.contiguous(), phi.imag.contiguous()
    assert _same(re, re.transpose(-1, -2).contiguous())
    assert torch.equal(im, -im.transpose(-1, -2)) and not torch.isnan(im).any()
    assert not torch.diagonal(im, dim1=-2, dim2=-1).any()


def _tab(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _poisoned(count):
    return torch.full((count + PAD,), float("nan"), dtype=torch.float32, device="cuda")


def _check_poison(buf, count, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[count:]).all(), "%s: the padding behind the result was written" % what
    assert not np.isnan(got[:count]).any(), "%s: an element of the result was not written" % what


def _raw_cov(Ys, Ms, complement):
    """pk2_bf_cov on lists of device tensors into a poisoned buffer -> complex64 (B, K', F, C, C)"""
    B, (Cn, _, F), K = len(Ys), Ys[0].shape, Ms[0].shape[0]
    KA = 2 if complement else K
    frames = (C.c_int32 * B)(*[y.shape[1] for y in Ys])
    L = _lib.lib()
    nbytes = L.pk2_bf_workspace_bytes(frames, B, Cn, F, K, int(complement))
    assert nbytes > 0
    work = torch.full((nbytes // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    count = B * KA * F * Cn * Cn * 2
    phi = _poisoned(count)
    masks = [m[k] for m in Ms for k in range(K)]
    _lib.check(L.pk2_bf_cov(_tab(Ys), _tab(masks), frames, B, Cn, F, K, int(complement), _lib.ptr(work), nbytes, _lib.ptr(phi),
                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(phi, count, "phi")
    assert np.isnan(work.cpu().numpy()[nbytes // 4:]).all(), "the workspace was written beyond its size"
    return torch.view_as_complex(phi[:count].view(B, KA, F, Cn, Cn, 2))


def _raw_weights(phi_s, phi_n, ref):
    """pk2_bf_mvdr_weights on lists of (F, C, C) tensors into poisoned buffers -> (w (B, F, C), ref_index, nonfinite)"""
    B, (F, Cn, _) = len(phi_s), phi_s[0].shape
    L = _lib.lib()
    nbytes = L.pk2_bf_workspace_bytes(None, B, Cn, F, 1, 0)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    count = B * F * Cn * 2
    w = _poisoned(count)
    idx = torch.full((B + PAD,), -7, dtype=torch.int32, device="cuda")
    flag = torch.full((B + PAD,), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.pk2_bf_mvdr_weights(_tab(phi_s), _tab(phi_n), B, Cn, F, _lib.BF_REF_SNR if ref == "snr" else ref, 1e-3,
                                     _lib.ptr(work), nbytes, _lib.ptr(w), _lib.ptr(idx), _lib.ptr(flag), _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(w, count, "w")
    assert (idx[B:] == -7).all() and (flag[B:] == -7).all() and (idx[:B] >= 0).all() and (flag[:B] >= 0).all()
    return torch.view_as_complex(w[:count].view(B, F, Cn, 2)), idx[:B], flag[:B]


def _raw_apply(Ys, ws):
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    frames = (C.c_int32 * B)(*[y.shape[1] for y in Ys])
    bufs = [_poisoned(y.shape[1] * F * 2) for y in Ys]
    _lib.check(_lib.lib().pk2_bf_apply(_tab(Ys), _tab(ws), frames, B, Cn, F, _tab(bufs), _lib.stream_ptr()))
    torch.cuda.synchronize()
    out = []
    for y, b in zip(Ys, bufs):
        _check_poison(b, y.shape[1] * F * 2, "X")
        out.append(torch.view_as_complex(b[:y.shape[1] * F * 2].view(y.shape[1], F, 2)))
    return out


@pytest.fixture(scope="module")
def want():
    """name -> dict(Y, masks, complement, phi, w, X) of the float64 restatement, computed once and left unchanged"""
    out = {}
    for name in list(R.CASES) + R.RAGGED:
        Y, m = R.case_inputs(name)
        comp = R.CASES[name][4] if name in R.CASES else True
        phi = R.covariance(Y, m, comp)
        w, _ = R.mvdr_weights(phi[0], phi[-1] if phi.shape[0] == 1 else phi[1], 0)
        wc = w.astype(np.complex64)
        out[name] = dict(Y=Y, masks=m, complement=comp, phi=phi, w=w, wc=wc, X=R.apply(Y, wc))
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_three_stages_match_the_restatement(name, want):
    c = want[name]
    Y, m = dev(c["Y"]), dev(c["masks"])
    phi = _raw_cov([Y], [m], c["complement"])[0]
    assert tuple(phi.shape) == c["phi"].shape
    got = phi.cpu().numpy()
    err = np.abs(got - c["phi"]).max() / np.abs(c["phi"]).max()
    print(name, "covariance rel err %.3e bound %.3e" % (err, COV_TOL))
    assert err <= COV_TOL
    # exactly Hermitian, real diagonal
    _assert_hermitian(phi)
    # the public function returns the same bits
    api = beamform.spatial_covariance(Y, m, complement=c["complement"])
    assert _same(api, phi)

    ps, pn = phi[0].contiguous(), (phi[1] if phi.shape[0] > 1 else phi[0]).contiguous()
    w, idx, flag = _raw_weights([ps], [pn], 0)
    err = np.abs(w[0].cpu().numpy() - c["w"]).max() / np.abs(c["w"]).max()
    print(name, "weights rel err %.3e bound %.3e" % (err, W_TOL))
    assert err <= W_TOL and idx.tolist() == [0] and flag.tolist() == [0]
    w_api, r_api = beamform.mvdr_weights(ps, pn, 0)
    assert _same(w_api, w[0]) and r_api.tolist() == [0] and beamform.last_nonfinite.tolist() == [0]
    if c["masks"].shape[0] == 1 and not c["masks"][0].any(axis=0).all():        # empty bins pass channel 0 through
        empty = ~c["masks"][0].any(axis=0)
        e0 = np.zeros(Y.shape[0], np.complex64)
        e0[0] = 1
        assert np.array_equal(w[0].cpu().numpy()[empty], np.tile(e0, (empty.sum(), 1)))

    wc = dev(c["wc"])
    X = _raw_apply([Y], [wc])[0]
    err = np.abs(X.cpu().numpy() - c["X"]).max() / np.abs(c["X"]).max()
    print(name, "apply rel err %.3e bound %.3e" % (err, APPLY_TOL))
    assert err <= APPLY_TOL
    assert _same(beamform.apply_weights(Y, wc), X)


def test_a_ragged_batch_equals_its_single_calls_bit_for_bit(want):
    Ys = [dev(want[n]["Y"]) for n in R.RAGGED]
    Ms = [dev(want[n]["masks"]) for n in R.RAGGED]
    assert [y.shape[1] for y in Ys] == R.RAGGED_FRAMES
    phi = _raw_cov(Ys, Ms, True)
    again = _raw_cov(Ys, Ms, True)
    assert _same(phi, again)
    ps, pn = [p[0].contiguous() for p in phi], [p[1].contiguous() for p in phi]
    for ref in (1, "snr"):
        w, idx, flag = _raw_weights(ps, pn, ref)
        w2, idx2, _ = _raw_weights(ps, pn, ref)
        assert _same(w, w2) and idx.tolist() == idx2.tolist() and flag.tolist() == [0] * 4
        X = _raw_apply(Ys, [x.contiguous() for x in w])
        X2 = _raw_apply(Ys, [x.contiguous() for x in w])
        for b, name in enumerate(R.RAGGED):
            one = _raw_cov([Ys[b]], [Ms[b]], True)
            assert _same(one[0], phi[b]), name
            w1, i1, _ = _raw_weights([ps[b]], [pn[b]], ref)
            assert _same(w1[0], w[b]) and i1.tolist() == [idx[b].item()], name
            assert _same(_raw_apply([Ys[b]], [w[b].contiguous()])[0], X[b]) and _same(X[b], X2[b]), name
            if ref == "snr":
                assert idx[b].item() == R.mvdr_weights(want[name]["phi"][0], want[name]["phi"][1], "snr")[1]
    # and against the restatement
    for b, name in enumerate(R.RAGGED):
        c = want[name]
        assert np.abs(phi[b].cpu().numpy() - c["phi"]).max() <= COV_TOL * np.abs(c["phi"]).max()
    # the list forms of the public functions make the same bits
    api = beamform.spatial_covariance(Ys, [m[0] for m in Ms], complement=True)
    assert all(_same(a, p) for a, p in zip(api, phi))
    w_api, r_api = beamform.mvdr_weights(ps, pn, "snr")
    assert all(_same(a, b) for a, b in zip(w_api, w)) and r_api.tolist() == idx.tolist()
    assert all(_same(a, b) for a, b in zip(beamform.apply_weights(Ys, w_api), X))


@pytest.mark.parametrize("name", R.SNR_CASES)
def test_snr_reference_matches_the_restatement(name, want):
    c = want[name]
    phi = _raw_cov([dev(c["Y"])], [dev(c["masks"])], c["complement"])[0]
    w, idx, _ = _raw_weights([phi[0].contiguous()], [phi[1].contiguous()], "snr")
    w_ref, r = R.mvdr_weights(c["phi"][0], c["phi"][1], "snr")
    assert idx.tolist() == [r]
    assert np.abs(w[0].cpu().numpy() - w_ref).max() <= W_TOL * np.abs(w_ref).max()
    fixed, _, _ = _raw_weights([phi[0].contiguous()], [phi[1].contiguous()], r)
    assert _same(fixed, w)


def test_a_tie_goes_to_the_lowest_channel():
    tie_s, tie_n = R.tie_covariances()
    w, idx, flag = _raw_weights([dev(tie_s)], [dev(tie_n)], "snr")
    assert idx.tolist() == [0] and flag.tolist() == [0]
    assert np.allclose(w[0].cpu().numpy(), np.tile(np.array([1 / 3, 0, 0], np.complex64), (tie_s.shape[0], 1)))


def test_non_finite_input_passes_the_reference_channel_and_raises_the_flag(want):
    c = want["c3_b0"]
    ps, pn = c["phi"][0].astype(np.complex64), c["phi"][1].astype(np.complex64)
    bad_s, bad_n = ps.copy(), pn.copy()
    bad_s[4, 1, 2] = np.nan
    bad_n[20, 0, 0] = np.inf
    w, idx, flag = _raw_weights([dev(ps), dev(bad_s), dev(bad_n)], [dev(pn), dev(pn), dev(pn)], 2)
    assert flag.tolist() == [0, 1, 1] and idx.tolist() == [2, 2, 2]
    w = w.cpu().numpy()
    e2 = np.array([0, 0, 1], np.complex64)
    assert np.array_equal(w[1, 4], e2) and np.array_equal(w[2, 20], e2)
    keep = np.ones(ps.shape[0], bool)
    keep[4] = False
    assert np.array_equal(w[1, keep], w[0, keep]) and np.isfinite(w).all()
    _, idx, flag = _raw_weights([dev(bad_s)], [dev(pn)], "snr")
    assert flag.tolist() == [1] and 0 <= idx.item() < 3


# ---------------------------------------------------------------------------------------------------------------------
# the beamformer end to end
# ---------------------------------------------------------------------------------------------------------------------
def _analyzer(F, **kw):
    return simulation.SpectrumAnalyzer(config=dict(R.CFGS[F], **kw))


@pytest.mark.parametrize("name", list(R.E2E_CASES))
def test_mask_beamformer_matches_the_restatement(name):
    F, Cn, n, seed = R.E2E_CASES[name]
    wav, mask = R.e2e_inputs(F, Cn, n, seed)
    want, ws, w_ref, _ = R.beamform(wav, mask, cfg=R.CFGS[F])
    bf = beamform.MaskBeamformer(_analyzer(F, do_dither=True))          # the analyzer's dither is not used
    got = bf(dev(wav), dev(mask))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n,) and got.is_cuda
    ok = ws >= 1e-3 * ws.max()
    err = np.abs(got.cpu().numpy() - want)[ok].max() / np.abs(want[ok]).max()
    print(name, "end to end rel err %.3e bound %.3e" % (err, E2E_TOL[name]))
    assert err <= E2E_TOL[name]
    assert tuple(bf.last_weights.shape) == (F, Cn) and bf.last_ref.tolist() == [0] and bf.last_ref.is_cuda
    assert bf.last_nonfinite.is_cuda and bf.last_nonfinite.tolist() == [0]
    assert np.abs(bf.last_weights.cpu().numpy() - w_ref).max() <= W_TOL * np.abs(w_ref).max()
    # an explicit noise mask (the two-mask kernel) stays within the bound; the batch form gives the single calls' bits
    two = bf(dev(wav), dev(mask), dev((1 - mask).astype(np.float32)))
    assert np.abs(two.cpu().numpy() - want)[ok].max() / np.abs(want[ok]).max() <= E2E_TOL[name]
    short = np.ascontiguousarray(wav[:, :n - 173])
    smask = np.ascontiguousarray(mask[:bf.analyzer.num_frames(n - 173)])
    outs = bf.batch([dev(wav), dev(short)], [dev(mask), dev(smask)])
    assert _same(outs[0], got) and _same(outs[1], bf(dev(short), dev(smask))) and tuple(outs[1].shape) == (n - 173,)


def test_it_is_a_beamformer_not_only_a_match():
    wav, target, mask = R.scene()
    got = beamform.MaskBeamformer(_analyzer(257))(dev(wav), dev(mask)).cpu().numpy()
    gain = R.scene_gain(got, wav, target)
    print("SI-SDR gain on the scene: %.2f dB (the restatement's: asserted >= 6 dB in the host test)" % gain)
    assert gain >= 3.0


# ---------------------------------------------------------------------------------------------------------------------
# SimulationPool with the data_config key
# ---------------------------------------------------------------------------------------------------------------------
def _pool(**extra):
    from pykaldi2_amd import data
    dc = dict(online_rir=True, use_reverb=True, use_dir_noise=True, simulation_prob=1.0, gain_norm=True)
    dc.update(extra)
    return data.SimulationPool.from_config({"synthetic": True, "data_config": dc})


def _utterance():
    from pykaldi2_amd import synth
    return synth.waveform(np.random.default_rng(3), 1.3)


def test_simulation_pool_with_the_key():
    pool, x = _pool(beamform={"n_mics": 4}), _utterance()
    np.random.seed(11)
    y = pool.maybe_simulate(x, DEV)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0],)
    assert torch.isfinite(y).all() and y.abs().max() > 0
    np.random.seed(11)
    y2 = pool.maybe_simulate(x, DEV)
    state = np.random.get_state()[1].copy()
    assert _same(y, y2)
    # the key adds no draw: the single-channel pool leaves numpy's generator in the same state
    np.random.seed(11)
    _pool().maybe_simulate(x, DEV)
    assert np.array_equal(np.random.get_state()[1], state)
    assert tuple(_pool(beamform=True).maybe_simulate(x, DEV).shape) == (x.shape[0],)      # the 7-channel default


def test_simulation_pool_without_the_key_is_the_unchanged_path():
    """maybe_simulate without the key against the single-channel steps written out as they were before the key existed"""
    pool, x = _pool(), _utterance()
    assert pool.beamform is None
    np.random.seed(12)
    got = pool.maybe_simulate(x, DEV)
    np.random.seed(12)
    xd = _lib.h2d(x, DEV)
    assert not np.random.random() > pool.prob
    noise = pool._on_device("n", int(np.random.choice(len(pool.noises))), DEV)[0]
    src_rir, noise_rir, delays = pool.online_rirs(2, DEV)
    want, _ = pool.sim(xd, [noise], src_rir, [noise_rir], normalize_gain=pool.gain_norm, rir_delays=delays)
    assert _same(got, want) and tuple(got.shape) == (x.shape[0],)


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    Y = torch.zeros(3, 5, 17, dtype=torch.complex64, device="cuda")
    m = torch.ones(5, 17, device="cuda")
    phi = torch.zeros(17, 3, 3, dtype=torch.complex64, device="cuda")
    w = torch.zeros(17, 3, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        beamform.spatial_covariance(torch.view_as_real(Y), m)
    with pytest.raises(ValueError, match="CUDA"):
        beamform.spatial_covariance(Y.cpu(), m)
    with pytest.raises(ValueError, match="at most 8"):
        beamform.spatial_covariance(torch.zeros(9, 5, 17, dtype=torch.complex64, device="cuda"), m)
    with pytest.raises(ValueError, match=r"\(N, F\) = \(5, 17\)"):
        beamform.spatial_covariance(Y, torch.ones(4, 17, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        beamform.spatial_covariance(Y, m.double())
    with pytest.raises(ValueError, match="float32"):
        beamform.spatial_covariance(Y, m.cpu())
    with pytest.raises(ValueError, match="1 to 4"):
        beamform.spatial_covariance(Y, [m] * 5)
    with pytest.raises(ValueError, match="complement"):
        beamform.spatial_covariance(Y, [m, m], complement=True)
    with pytest.raises(ValueError, match="first one"):
        beamform.spatial_covariance([Y, Y[:2].contiguous()], [m, m])
    for ref in (3, -1, "best", 1.0):
        with pytest.raises(ValueError, match="ref"):
            beamform.mvdr_weights(phi, phi, ref)
    with pytest.raises(ValueError, match="diag_load"):
        beamform.mvdr_weights(phi, phi, 0, diag_load=-1)
    with pytest.raises(ValueError, match="complex64"):
        beamform.mvdr_weights(phi, phi.cpu())
    with pytest.raises(ValueError, match="must both be"):
        beamform.mvdr_weights(phi, phi[:16].contiguous())
    with pytest.raises(ValueError, match=r"\(F, C\) = \(17, 3\)"):
        beamform.apply_weights(Y, w[:, :2].contiguous())
    with pytest.raises(ValueError, match="complex64"):
        beamform.apply_weights(Y, w.cpu())
    bf = beamform.MaskBeamformer(_analyzer(17))
    with pytest.raises(ValueError, match="at most 8"):
        bf(torch.zeros(9, 100, device="cuda"), m)
    with pytest.raises(ValueError, match="float32"):
        bf(torch.zeros(3, 100, dtype=torch.float64, device="cuda"), m)
    with pytest.raises(ValueError, match=r"\(N, F\)"):
        bf(torch.zeros(3, 100, device="cuda"), m)        # 100 samples are 10 frames, the mask has 5
    with pytest.raises(ValueError, match="outside the 3 channels"):
        beamform.MaskBeamformer(_analyzer(17), ref=5)(torch.zeros(3, 100, device="cuda"), torch.ones(10, 17, device="cuda"))
