"""pykaldi2_amd.cgmm on the device against the float64 restatement tests/cgmm_ref.py: every stage given the restatement's
inputs, the whole EM after 1, 3 and 10 iterations, poisoned buffers with checked padding, exact Hermitian symmetry, batch
independence and run-to-run identity bit for bit, the class order, the non-finite flag, the beamformer with the estimator
end to end, SimulationPool with `mask: cgmm`, and bin/dump_loglikes.py -array_frontend."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_ref as BR  # noqa: E402
import cgmm_ref as R  # noqa: E402

from pykaldi2_amd import _lib, beamform, cgmm, simulation  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# float32 kernels against the float64 restatement.  The rule: run the restatement's float32 mode on the CPU
# against its float64 result over these very cases (R.CASES and R.RAGGED) and take 4 x the largest error; masks are absolute
# errors, the rest is relative to max|want|.  Measured with `python tests/cgmm_ref.py`, never with the device:
INIT_TOL = 4 * 2.17e-7        # start state R (the largest over the cases; the smallest is 1.9e-8, C = 1 and one frame)
INIT_LA_TOL = 4 * 1.26e-7     # start state log alpha: 2.7e-9 (log 1/2, rounded) .. 1.26e-7
LINV_TOL = 4 * 3.84e-8        # L^-1, factored in float64 and rounded once: 1.2e-12 (guided: |L^-1| = 1e5 on the zero bins) .. 3.84e-8
BIAS_TOL = 4 * 5.23e-8        # b: 2.98e-8 .. 5.23e-8
LAM_TOL = 4 * 3.81e-6         # posteriors of one E-step (absolute): 0 (C = 1) .. 3.81e-6
PHI_TOL = 4 * 1.27e-7         # phi: 5.5e-8 .. 1.27e-7
LL1_TOL = 4 * 2.55e-8         # log-likelihood of one E-step: 4.4e-11 .. 2.55e-8
UPDATE_TOL = 4 * 2.99e-7      # R of one M-step: 6.6e-8 .. 2.99e-7
LA_TOL = 4 * 2.50e-7          # log alpha of one M-step: 2.7e-9 .. 2.50e-7
MASK_TOL = 4 * 9.39e-5        # masks after 1, 3 and 10 iterations (absolute): 0 (C = 1) .. 9.39e-5
COV_TOL = 4 * 1.88e-4         # last_cov after 1, 3 and 10 iterations: 2.9e-7 .. 1.88e-4
LA_EM_TOL = 4 * 1.71e-5       # log alpha after 1, 3 and 10 iterations: 2.7e-9 .. 1.71e-5
LL_TOL = 4 * 9.16e-8          # LL per iteration: 1.5e-9 .. 9.16e-8
# MaskBeamformer(mask_estimator=CgmmMaskEstimator) on the RIR scene: SI-SDR gain over channel 0 of the restatement
# (R.enhance on R.rir_scene, float64, measured on the CPU with `python tests/cgmm_ref.py`)
REF_GAIN_DB = 5.68
PAD = 64                      # poisoned elements behind every output
DEV = torch.device("cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _assert_hermitian(phi):
    re, im = phi.real.contiguous(), phi.imag.contiguous()
    assert _same(re, re.transpose(-1, -2).contiguous())
    assert torch.equal(im, -im.transpose(-1, -2)) and not torch.isnan(im).any()
    assert not torch.diagonal(im, dim1=-2, dim2=-1).any()


def _tab(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _opt_tab(tensors):
    return None if tensors is None else _tab(tensors)


def _poisoned(count, dtype=torch.float32):
    return torch.full((count + PAD,), float("nan"), dtype=dtype, device="cuda")


def _check_poison(buf, count, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[count:]).all(), "%s: the padding behind the result was written" % what
    assert not np.isnan(got[:count]).any(), "%s: an element of the result was not written" % what


def _ints(count):
    return torch.full((count + PAD,), -7, dtype=torch.int32, device="cuda")


def _check_ints(buf, count, what):
    assert (buf[count:] == -7).all() and ((buf[:count] == 0) | (buf[:count] == 1)).all(), what


def _work(Ys, K):
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    frames = (C.c_int32 * B)(*[y.shape[1] for y in Ys])
    nbytes = _lib.lib().pk2_cgmm_workspace_bytes(frames, B, Cn, F, K)
    assert nbytes > 0 and nbytes % 4 == 0
    return frames, torch.full((nbytes // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda"), nbytes


def _check_work(work, nbytes):
    assert np.isnan(work[nbytes // 4:].cpu().numpy()).all(), "the workspace was written beyond its size"


def _raw_state(fn, Ys, K, *tables):
    """pk2_cgmm_init / pk2_cgmm_update into poisoned buffers -> (R complex64 (B, K, F, C, C), log_alpha (B, K, F))"""
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    frames, work, nbytes = _work(Ys, K)
    nR, nla = B * K * F * Cn * Cn * 2, B * K * F
    Rb, la = _poisoned(nR), _poisoned(nla)
    _lib.check(fn(_tab(Ys), *[_opt_tab(t) for t in tables], frames, B, Cn, F, K, _lib.ptr(work), nbytes, _lib.ptr(Rb), _lib.ptr(la),
                  _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(Rb, nR, "R")
    _check_poison(la, nla, "log_alpha")
    _check_work(work, nbytes)
    return torch.view_as_complex(Rb[:nR].view(B, K, F, Cn, Cn, 2)), la[:nla].view(B, K, F)


def _raw_init(Ys, inits, acts, K):
    return _raw_state(_lib.lib().pk2_cgmm_init, Ys, K, inits, acts)


def _raw_update(Ys, lams, phis, acts, K):
    return _raw_state(_lib.lib().pk2_cgmm_update, Ys, K, lams, phis, acts)


def _raw_factor(Rk, la, diag_load=1e-3):
    """R (B, K, F, C, C), la (B, K, F) -> (linv (B, K, C (C + 1), F), bias (B, K, F), bad (B, K, F), nonfinite (B,))"""
    B, K, F, Cn, _ = Rk.shape
    nl, nb = B * K * Cn * (Cn + 1) * F, B * K * F
    linv, bias, bad, flag = _poisoned(nl), _poisoned(nb), _ints(nb), _ints(B)
    _lib.check(_lib.lib().pk2_cgmm_factor(_lib.ptr(Rk.contiguous()), _lib.ptr(la.contiguous()), B, Cn, F, K, diag_load,
                                          _lib.ptr(linv), _lib.ptr(bias), _lib.ptr(bad), _lib.ptr(flag), _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(linv, nl, "linv")
    _check_poison(bias, nb, "bias")
    _check_ints(bad, nb, "bad")
    _check_ints(flag, B, "nonfinite")
    return linv[:nl].view(B, K, Cn * (Cn + 1), F), bias[:nb].view(B, K, F), bad[:nb].view(B, K, F), flag[:B]


def _raw_posteriors(Ys, acts, linv, bias, bad):
    B, (Cn, _, F), K = len(Ys), Ys[0].shape, bias.shape[1]
    frames, work, nbytes = _work(Ys, K)
    counts = [K * y.shape[1] * F for y in Ys]
    lam, phi = [_poisoned(n) for n in counts], [_poisoned(n) for n in counts]
    ll = _poisoned(B, torch.float64)
    _lib.check(_lib.lib().pk2_cgmm_posteriors(_tab(Ys), _opt_tab(acts), frames, B, Cn, F, K, _lib.ptr(linv.contiguous()),
                                              _lib.ptr(bias.contiguous()), _lib.ptr(bad.contiguous()), _lib.ptr(work), nbytes,
                                              _tab(lam), _tab(phi), _lib.ptr(ll), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for n, a, b in zip(counts, lam, phi):
        _check_poison(a, n, "lam")
        _check_poison(b, n, "phi")
    _check_poison(ll, B, "ll")
    _check_work(work, nbytes)
    shape = [(K, y.shape[1], F) for y in Ys]
    return [a[:n].view(s) for a, n, s in zip(lam, counts, shape)], [b[:n].view(s) for b, n, s in zip(phi, counts, shape)], ll[:B]


def _raw_cgmm(Ys, inits, acts, K, iters, purity, diag_load=1e-3, finite=True):
    """pk2_cgmm into poisoned buffers -> (masks [(K, N, F)], R (B, K, F, C, C), log_alpha (B, K, F), ll (B, iters), flag (B,)).
    finite=False: the input holds a NaN, which its bin's R keeps, so R is only checked for its padding."""
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    frames, work, nbytes = _work(Ys, K)
    counts = [K * y.shape[1] * F for y in Ys]
    masks = [_poisoned(n) for n in counts]
    nR, nla = B * K * F * Cn * Cn * 2, B * K * F
    Rb, la, ll, flag = _poisoned(nR), _poisoned(nla), _poisoned(B * iters, torch.float64), _ints(B)
    _lib.check(_lib.lib().pk2_cgmm(_tab(Ys), _opt_tab(inits), _opt_tab(acts), frames, B, Cn, F, K, iters, diag_load, int(purity),
                                   _lib.ptr(work), nbytes, _tab(masks), _lib.ptr(Rb), _lib.ptr(la), _lib.ptr(ll), _lib.ptr(flag),
                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    for n, m in zip(counts, masks):
        _check_poison(m, n, "masks")
    if finite:
        _check_poison(Rb, nR, "R")
    else:
        assert torch.isnan(Rb[nR:]).all(), "R: the padding behind the result was written"
    _check_poison(la, nla, "log_alpha")
    _check_poison(ll, B * iters, "ll")
    _check_ints(flag, B, "nonfinite")
    _check_work(work, nbytes)
    return ([m[:n].view(K, y.shape[1], F) for m, n, y in zip(masks, counts, Ys)],
            torch.view_as_complex(Rb[:nR].view(B, K, F, Cn, Cn, 2)), la[:nla].view(B, K, F), ll[:B * iters].view(B, iters), flag[:B])


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def want():
    """name -> the restatement's stages (R.stages) and its whole EM with the snapshots after 1, 3 and 10 iterations, in the
    order 'keep' (the class order is a test of its own); computed once and left unchanged"""
    out = {}
    for name in list(R.CASES) + R.RAGGED:
        s = R.stages(name)
        s["em"] = R.em(s["Y"], 10, s["init"], s["act"], order="keep", snapshots=R.SNAPSHOTS)
        out[name] = s
    return out


def _inputs(s):
    Y = dev(s["Y"])
    init = None if s["init"] is None else [dev(s["init"])]
    act = None if s["act"] is None else [dev(s["act"])]
    K = 2 if s["init"] is None else s["init"].shape[0]
    return Y, init, act, K


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_stage_matches_the_restatement(name, want):
    s = want[name]
    Y, init, act, K = _inputs(s)
    Cn = Y.shape[0]
    one = lambda x: None if x is None else x[0]      # noqa: E731

    R0, la0 = _raw_init([Y], init, act, K)
    e = _rel(R0[0].cpu().numpy(), s["R0"]), _rel(la0[0].cpu().numpy(), s["la0"])
    print(name, "init rel err %.3e (bound %.3e), log alpha %.3e (bound %.3e)" % (e[0], INIT_TOL, e[1], INIT_LA_TOL))
    assert e[0] <= INIT_TOL and e[1] <= INIT_LA_TOL
    _assert_hermitian(R0)
    api = cgmm.cgmm_init(Y, one(init), one(act))
    assert _same(api[0], R0[0]) and _same(api[1], la0[0])

    linv, bias, bad, flag = _raw_factor(dev(s["R32"])[None], dev(s["la32"])[None])
    e = _rel(R.unpack_linv(linv[0].cpu().numpy(), Cn), s["Li"]), _rel(bias[0].cpu().numpy(), s["b"])
    print(name, "factor rel err %.3e (bound %.3e), bias %.3e (bound %.3e)" % (e[0], LINV_TOL, e[1], BIAS_TOL))
    assert e[0] <= LINV_TOL and e[1] <= BIAS_TOL
    assert not bad.any() and flag.tolist() == [0] and not s["bad"].any()
    fac = cgmm.cgmm_factor(dev(s["R32"]), dev(s["la32"]))
    assert _same(fac[0], linv[0]) and _same(fac[1], bias[0]) and _same(fac[2], bad[0]) and cgmm.last_nonfinite.tolist() == [0]

    linv_in, bias_in = dev(R.pack_linv(s["Li32"]))[None], dev(s["b32"])[None]
    bad_in = torch.zeros(1, K, Y.shape[2], dtype=torch.int32, device="cuda")
    lam, phi, ll = _raw_posteriors([Y], act, linv_in, bias_in, bad_in)
    e = (float(np.abs(lam[0].cpu().numpy() - s["lam"]).max()), _rel(phi[0].cpu().numpy(), s["phi"]),
         abs(ll[0].item() - s["ll"]) / abs(s["ll"]))
    print(name, "posteriors abs err %.3e (bound %.3e), phi %.3e (bound %.3e), ll %.3e (bound %.3e)"
          % (e[0], LAM_TOL, e[1], PHI_TOL, e[2], LL1_TOL))
    assert e[0] <= LAM_TOL and e[1] <= PHI_TOL and e[2] <= LL1_TOL
    api = cgmm.cgmm_posteriors(Y, (linv_in[0], bias_in[0], bad_in[0]), one(act))
    assert _same(api[0], lam[0]) and _same(api[1], phi[0]) and _same(api[2], ll[0]) and api[2].dtype == torch.float64

    lam_in, phi_in = dev(s["lam32"]), dev(s["phi32"])
    Ru, lau = _raw_update([Y], [lam_in], [phi_in], act, K)
    e = _rel(Ru[0].cpu().numpy(), s["Ru"]), _rel(lau[0].cpu().numpy(), s["lau"])
    print(name, "update rel err %.3e (bound %.3e), log alpha %.3e (bound %.3e)" % (e[0], UPDATE_TOL, e[1], LA_TOL))
    assert e[0] <= UPDATE_TOL and e[1] <= LA_TOL
    _assert_hermitian(Ru)
    api = cgmm.cgmm_update(Y, lam_in, phi_in, one(act))
    assert _same(api[0], Ru[0]) and _same(api[1], lau[0])


@pytest.mark.parametrize("iters", R.SNAPSHOTS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_whole_em_matches_the_restatement(name, iters, want):
    s = want[name]
    Y, init, act, K = _inputs(s)
    masks, Rk, la, ll, flag = _raw_cgmm([Y], init, act, K, iters, False)
    w_masks, w_R, w_la, _ = s["em"]["snap"][iters]
    e = (float(np.abs(masks[0].cpu().numpy() - w_masks).max()), _rel(Rk[0].cpu().numpy(), w_R),
         _rel(ll[0].cpu().numpy(), s["em"]["ll"][:iters]))
    print(name, iters, "masks abs err %.3e (bound %.3e), cov %.3e (bound %.3e), LL %.3e (bound %.3e)"
          % (e[0], MASK_TOL, e[1], COV_TOL, e[2], LL_TOL))
    assert e[0] <= MASK_TOL and e[1] <= COV_TOL and e[2] <= LL_TOL
    assert _rel(la[0].cpu().numpy(), w_la) <= LA_EM_TOL
    assert flag.tolist() == [0]
    _assert_hermitian(Rk)
    m = masks[0]
    live = torch.ones(Y.shape[1], dtype=torch.bool) if s["act"] is None else torch.from_numpy((s["act"] > 0).any(axis=0))
    assert (m[:, live].sum(dim=0) - 1).abs().max() <= 1e-6 and not m[:, ~live].any()
    # the public function returns the same bits, and keeps the likelihoods, the covariances and the flag on the device
    one = lambda x: None if x is None else x[0]      # noqa: E731
    api = cgmm.cgmm_masks(Y, K, iters, one(init), one(act), order="keep")
    assert _same(api, m) and _same(cgmm.last_cov, Rk[0]) and _same(cgmm.last_ll, ll[0]) and _same(cgmm.last_log_alpha, la[0])
    assert cgmm.last_ll.is_cuda and cgmm.last_ll.dtype == torch.float64 and tuple(cgmm.last_ll.shape) == (iters,)
    assert cgmm.last_nonfinite.is_cuda and cgmm.last_nonfinite.tolist() == [0]


def test_a_ragged_batch_equals_its_single_calls_bit_for_bit(want):
    Ys = [dev(want[n]["Y"]) for n in R.RAGGED]
    assert [y.shape[1] for y in Ys] == R.RAGGED_FRAMES
    got = _raw_cgmm(Ys, None, None, 2, 5, True)
    again = _raw_cgmm(Ys, None, None, 2, 5, True)
    for a, b in zip(got[0], again[0]):
        assert _same(a, b)
    assert all(_same(a, b) for a, b in zip(got[1:], again[1:]))
    for b, name in enumerate(R.RAGGED):
        one = _raw_cgmm([Ys[b]], None, None, 2, 5, True)
        assert _same(one[0][0], got[0][b]) and _same(one[1][0], got[1][b]) and _same(one[2][0], got[2][b]), name
        assert _same(one[3][0], got[3][b]) and one[4].tolist() == [0], name
        w = want[name]["em"]
        assert _rel(got[3][b].cpu().numpy(), w["ll"][:5]) <= LL_TOL
    # the list forms of the public functions make the same bits
    api = cgmm.cgmm_masks(Ys, iterations=5)
    assert all(_same(a, m) for a, m in zip(api, got[0])) and all(_same(a, r) for a, r in zip(cgmm.last_cov, got[1]))
    assert _same(cgmm.last_ll, got[3]) and cgmm.last_nonfinite.tolist() == [0] * 4
    R0, la0 = cgmm.cgmm_init(Ys)
    fac = cgmm.cgmm_factor(R0, la0)
    lam, phi, ll = cgmm.cgmm_posteriors(Ys, fac)
    Rn, lan = cgmm.cgmm_update(Ys, lam, phi)
    first = _raw_cgmm(Ys, None, None, 2, 1, False)
    assert all(_same(a, m) for a, m in zip(lam, first[0])) and all(_same(a, r) for a, r in zip(Rn, first[1]))
    assert all(_same(a, r) for a, r in zip(lan, first[2])) and _same(ll, first[3][:, 0])


def test_35_utterances_take_two_launches_per_stage(want):
    names = [R.RAGGED[i % 4] for i in range(35)]
    Ys = [dev(want[n]["Y"]) for n in names]
    masks, Rk, la, ll, flag = _raw_cgmm(Ys, None, None, 2, 2, True)
    single = {n: _raw_cgmm([dev(want[n]["Y"])], None, None, 2, 2, True) for n in R.RAGGED}
    for b, n in enumerate(names):
        one = single[n]
        assert _same(masks[b], one[0][0]) and _same(Rk[b], one[1][0]) and _same(la[b], one[2][0]) and _same(ll[b], one[3][0]), b
    assert flag.tolist() == [0] * 35


# (C, K, N, F).  (3, 2, 33, 65): the second 32-frame part holds one frame, the second 64-bin tile one lane.
# (8, 4, 98, 17): the one instantiation that keeps sums in AGPRs; four parts, the last short.
@pytest.mark.parametrize("shape", [(3, 2, 33, 65), (8, 4, 98, 17)])
def test_the_m_step_with_phi_one_is_the_masked_covariance_bit_for_bit(shape):
    """The M-step and the beamformer's covariances are one pass (csrc/array_internal.h) under two weights: with phi = 1 the
    weight lam / 1.0f is lam exactly, the normaliser is the same float32 chain and the reduce the same float64 sum."""
    Cn, K, N, F = shape
    g = torch.Generator().manual_seed(1234 + Cn)
    Y = torch.complex(torch.randn(Cn, N, F, generator=g), torch.randn(Cn, N, F, generator=g)).cuda()
    lam = (torch.rand(K, N, F, generator=g) * 0.998 + 0.001).cuda()      # in (0, 1); need not sum to one over the classes
    Rk, _ = cgmm.cgmm_update(Y, lam, torch.ones_like(lam))
    phi = beamform.spatial_covariance(Y, lam)
    assert tuple(Rk.shape) == (K, F, Cn, Cn) and torch.isfinite(torch.view_as_real(Rk)).all()
    assert torch.equal(Rk, phi)


@pytest.mark.parametrize("name", [n for n in list(R.CASES) + R.RAGGED if R._shape(n)[3] == 2 and R._shape(n)[0] > 1])
def test_the_class_order_matches_the_restatement(name, want):
    """on the bins whose purities differ by >= 1 % in the restatement (most bins: the host test)"""
    s = want[name]
    Y = dev(s["Y"])
    keep = _raw_cgmm([Y], None, None, 2, 10, False)
    pure = _raw_cgmm([Y], None, None, 2, 10, True)
    p = R.purity(s["em"]["R"])
    clear = np.abs(p[1] - p[0]) >= 0.01 * np.maximum(p[0], p[1])
    swap = torch.from_numpy((p[1] > p[0]) & clear)
    stay = torch.from_numpy(~(p[1] > p[0]) & clear)
    assert clear.mean() >= 0.9
    for k_ in (keep, pure):
        assert k_[4].tolist() == [0]
    (mk, Rk, lk), (mp, Rp, lp) = [(x[0][0], x[1][0], x[2][0]) for x in (keep, pure)]
    assert _same(mp[:, :, stay], mk[:, :, stay]) and _same(Rp[:, stay], Rk[:, stay]) and _same(lp[:, stay], lk[:, stay])
    assert _same(mp[:, :, swap], mk.flip(0)[:, :, swap]) and _same(Rp[:, swap], Rk.flip(0)[:, swap])
    assert _same(lp[:, swap], lk.flip(0)[:, swap])
    # every bin is one or the other, bit for bit
    same = (mp == mk).all(dim=0).all(dim=0)
    flipped = (mp == mk.flip(0)).all(dim=0).all(dim=0)
    assert (same | flipped).all()


def test_a_tie_keeps_the_order():
    """Two classes that start identical stay identical bit for bit (equal l_k give lam = 1/2 exactly), so their purities
    are equal in every bin: the purity order must change nothing."""
    r = np.random.RandomState(3)
    Y = dev((r.standard_normal((3, 40, 17)) + 1j * r.standard_normal((3, 40, 17))).astype(np.complex64))
    init = dev(np.full((2, 40, 17), 0.5, np.float32))          # both classes start, and stay, identical
    keep = _raw_cgmm([Y], [init], None, 2, 3, False)
    pure = _raw_cgmm([Y], [init], None, 2, 3, True)
    assert _same(keep[1][0, 0], keep[1][0, 1])                 # a tie in every bin
    assert _same(pure[0][0], keep[0][0]) and _same(pure[1], keep[1]) and _same(pure[2], keep[2])
    with pytest.raises(ValueError, match="two classes"):
        cgmm.cgmm_masks(Y, 3, init=dev(np.full((3, 40, 17), 1 / 3, np.float32)), order="purity")


def test_a_bad_bin_gets_uniform_masks_and_raises_the_flag(want):
    s = want["r0"]
    bad = s["Y"].copy()
    bad[1, 4, 7] = np.nan
    inf = s["Y"].copy()
    inf[0, 0, 20] = np.inf
    Ys = [dev(s["Y"]), dev(bad), dev(inf)]
    masks, Rk, la, ll, flag = _raw_cgmm(Ys, None, None, 2, 3, True, finite=False)
    assert flag.tolist() == [0, 1, 1]
    assert torch.isfinite(torch.view_as_real(Rk[0])).all() and torch.isfinite(torch.view_as_real(Rk[1][:, [6, 8]])).all()
    assert (masks[1][:, :, 7] == 0.5).all() and (masks[2][:, :, 20] == 0.5).all()
    keep = torch.ones(33, dtype=torch.bool)
    keep[7] = False
    assert _same(masks[1][:, :, keep], masks[0][:, :, keep]) and torch.isfinite(masks[1]).all()
    assert torch.isfinite(ll).all()
    w = R.em(bad, 3)
    assert w["nonfinite"] and abs(ll[1, 2].item() - w["ll"][2]) <= LL_TOL * abs(w["ll"][2])
    # the stage function reports the class and the bin
    Rbad = dev(s["R32"]).clone()
    Rbad[1, 5, 0, 0] = -1.0          # not positive definite
    fac = cgmm.cgmm_factor(Rbad, dev(s["la32"]))
    assert cgmm.last_nonfinite.tolist() == [1] and fac[2].sum().item() == 1 and fac[2][1, 5].item() == 1
    lam, _, _ = cgmm.cgmm_posteriors(Ys[0], fac)
    assert (lam[:, :, 5] == 0.5).all() and not (lam[:, :, 4] == 0.5).all()


# ---------------------------------------------------------------------------------------------------------------------
# the beamformer with the estimator, end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_beamformer_with_the_estimator_enhances_a_rir_scene():
    rir = np.load(os.path.join(ROOT, "tests", "golden", R.GOLDEN_RIR))
    wav, target = R.rir_scene(rir)
    analyzer = simulation.SpectrumAnalyzer(do_dither=False)
    est = cgmm.CgmmMaskEstimator(analyzer)
    bf = beamform.MaskBeamformer(analyzer, mask_estimator=est)
    got = bf(dev(wav))
    assert got.dtype == torch.float32 and tuple(got.shape) == (wav.shape[1],)
    gain = BR.scene_gain(got.cpu().numpy(), wav, target)
    print("SI-SDR gain on the RIR scene: %.2f dB (the restatement's: %r dB)" % (gain, REF_GAIN_DB))
    assert gain >= REF_GAIN_DB - 0.5 and gain >= 3.0
    assert est.last_nonfinite.tolist() == [0] and bf.last_nonfinite.tolist() == [0] and tuple(est.last_cov[0].shape) == (2, 257, 4, 4)
    # masks that are passed in are used as before, whatever the estimator
    speech, noise = est(dev(wav))
    assert _same(bf(dev(wav), speech, noise), got)
    plain = beamform.MaskBeamformer(analyzer)
    assert _same(plain(dev(wav), speech, noise), got)
    with pytest.raises(ValueError, match="no speech mask"):
        plain(dev(wav))
    outs = bf.batch([dev(wav), dev(np.ascontiguousarray(wav[:, :9000]))])
    assert _same(outs[0], got) and tuple(outs[1].shape) == (9000,)


# ---------------------------------------------------------------------------------------------------------------------
# SimulationPool with `mask: cgmm`, and the decoding front end
# ---------------------------------------------------------------------------------------------------------------------
def _pool(**extra):
    from pykaldi2_amd import data
    dc = dict(online_rir=True, use_reverb=True, use_dir_noise=True, simulation_prob=1.0, gain_norm=True)
    dc.update(extra)
    return data.SimulationPool.from_config({"synthetic": True, "data_config": dc})


def test_simulation_pool_with_estimated_masks_draws_what_the_ideal_mask_draws():
    from pykaldi2_amd import synth
    x = synth.waveform(np.random.default_rng(3), 1.3)
    states, outs = [], []
    for extra in (dict(beamform={"n_mics": 4, "mask": "cgmm", "cgmm_iterations": 4}),
                  dict(beamform={"n_mics": 4, "mask": "cgmm", "cgmm_iterations": 4}, wpe={"taps": 4}),
                  dict(beamform={"n_mics": 4, "mask": "ideal"}), dict(beamform={"n_mics": 4})):
        pool = _pool(**extra)
        np.random.seed(11)
        y = pool.maybe_simulate(x, DEV)
        states.append(np.random.get_state()[1].copy())
        assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0],)
        assert torch.isfinite(y).all() and y.abs().max() > 0
        outs.append(y)
    assert all(np.array_equal(s, states[0]) for s in states[1:])
    assert _same(outs[2], outs[3])                     # `mask: ideal` is the path without the key
    assert not _same(outs[0], outs[2]) and not _same(outs[0], outs[1])
    np.random.seed(11)
    assert _same(_pool(beamform={"n_mics": 4, "mask": "cgmm", "cgmm_iterations": 4}).maybe_simulate(x, DEV), outs[0])


def test_dump_loglikes_with_the_array_front_end(tmp_path):
    from pykaldi2_amd import data, fbank, kaldi_io
    import yaml
    cfg = dict(data_config=dict(simulation_prob=0),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    cfg_path, ark = str(tmp_path / "cfg.yaml"), str(tmp_path / "out.ark")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "dump_loglikes.py"), "-config", cfg_path, "-synthetic", "2",
                          "-array_frontend", "wpe_mvdr", "-out_file", ark], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    source = data.SyntheticSource(120, seed=11)
    utts = [source.draw() for _ in range(2)]
    got = dict(kaldi_io.read_matrix_ark(ark))
    assert sorted(got) == sorted(u[3] for u in utts)
    for u in utts:
        m = got[u[3]]
        assert m.shape == (fbank.num_frames(u[0].shape[0]), 120) and np.isfinite(m).all()


def test_argument_errors():
    Y = torch.zeros(3, 5, 17, dtype=torch.complex64, device="cuda")
    m3 = torch.full((3, 5, 17), 1 / 3, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        cgmm.cgmm_masks(torch.view_as_real(Y))
    with pytest.raises(ValueError, match="CUDA"):
        cgmm.cgmm_masks(Y.cpu())
    with pytest.raises(ValueError, match="at most 8"):
        cgmm.cgmm_masks(torch.zeros(9, 5, 17, dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="first one"):
        cgmm.cgmm_masks([Y, Y[:2].contiguous()])
    with pytest.raises(ValueError, match="num_classes"):
        cgmm.cgmm_masks(Y, 5)
    with pytest.raises(ValueError, match="need init"):
        cgmm.cgmm_masks(Y, 3)
    with pytest.raises(ValueError, match="init has 3 masks"):
        cgmm.cgmm_masks(Y, 2, init=m3)
    with pytest.raises(ValueError, match=r"\(K, N, F\)"):
        cgmm.cgmm_masks(Y, 3, init=m3[:, :4].contiguous())
    with pytest.raises(ValueError, match="float32"):
        cgmm.cgmm_masks(Y, 3, init=m3.double())
    with pytest.raises(ValueError, match="iterations"):
        cgmm.cgmm_masks(Y, iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        cgmm.cgmm_masks(Y, iterations=33)
    with pytest.raises(ValueError, match="diag_load"):
        cgmm.cgmm_masks(Y, diag_load=-1)
    with pytest.raises(ValueError, match="order"):
        cgmm.cgmm_masks(Y, order="best")
    with pytest.raises(ValueError, match="two classes"):
        cgmm.cgmm_masks(Y, 3, init=m3, order="purity")
    with pytest.raises(ValueError, match=r"\(K, N\) = \(2, 5\)"):
        cgmm.cgmm_masks(Y, activity=torch.ones(2, 4, device="cuda"))
    with pytest.raises(ValueError, match="activity"):
        cgmm.cgmm_masks(Y, activity=torch.ones(2, 5))
    with pytest.raises(ValueError, match="entries of init"):
        cgmm.cgmm_masks([Y, Y], 3, init=[m3])
    with pytest.raises(ValueError, match="factor"):
        cgmm.cgmm_posteriors(Y, (m3, m3))
    with pytest.raises(ValueError, match="log_alpha"):
        cgmm.cgmm_factor(torch.zeros(2, 17, 3, 3, dtype=torch.complex64, device="cuda"), torch.zeros(2, 16, device="cuda"))
    with pytest.raises(ValueError, match="phi"):
        cgmm.cgmm_update(Y, m3, m3[:2].contiguous())
    est = cgmm.CgmmMaskEstimator(simulation.SpectrumAnalyzer(config=BR.CFGS[17]))
    with pytest.raises(ValueError, match="at most 8"):
        est(torch.zeros(9, 100, device="cuda"))
