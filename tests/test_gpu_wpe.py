"""pykaldi2_amd.dereverb on the device against the float64 restatement tests/wpe_ref.py: every stage at the shapes where it
can go wrong, poisoned padding, exact-integer correlations and exact Hermitian symmetry bit for bit, the solve's residual,
batch independence and run-to-run identity, the non-finite pass-through, the Dereverberator, the late-reverberation scene
and SimulationPool with the data_config key."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wpe_ref as R  # noqa: E402

from pykaldi2_amd import _lib, dereverb, simulation  # noqa: E402

pytestmark = pytest.mark.gpu

# float32 kernels against the float64 restatement.  The rule: run the restatement in its float32 mode on the
# CPU against its float64 result over these very cases (R.CASES and R.RAGGED) and take 4 x the largest error relative to
# max|want|.  Measured with `python tests/wpe_ref.py` (wpe_ref.float32_errors), never with the device:
POWER_TOL = 4 * 1.49e-7      # power(float32): 6.00e-9 .. 1.49e-7
CORR_TOL = 4 * 1.28e-6       # correlations(float32), the larger of R and P: 0 (N <= delay) .. 1.28e-6
APPLY_TOL = 4 * 9.23e-7      # apply(float32) with the complex64 G: 0 (N <= delay) .. 9.23e-7
WPE_TOL = 4 * 2.31e-4        # three iterations in float32 mode against all-float64: 0 (N <= delay) .. 2.31e-4; the condition
#                              on the inputs, every case below 1e-3, is asserted in tests/test_wpe_host.py
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


def _frames(Ys):
    return (C.c_int32 * len(Ys))(*[y.shape[1] for y in Ys])


def _poisoned(count):
    return torch.full((count + PAD,), float("nan"), dtype=torch.float32, device="cuda")


def _check_poison(buf, count, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[count:]).all(), "%s: the padding behind the result was written" % what
    assert not np.isnan(got[:count]).any(), "%s: an element of the result was not written" % what


def _work(Ys, taps, delay):
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    nbytes = _lib.lib().pk2_wpe_workspace_bytes(_frames(Ys), B, Cn, F, taps, delay)
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda"), nbytes


def _check_work(work, nbytes):
    assert np.isnan(work[nbytes // 4:].cpu().numpy()).all(), "the workspace was written beyond its size"


def _raw_power(Ys):
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    bufs = [_poisoned(y.shape[1] * F) for y in Ys]
    _lib.check(_lib.lib().pk2_wpe_power(_tab(Ys), _frames(Ys), B, Cn, F, _tab(bufs), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for y, b in zip(Ys, bufs):
        _check_poison(b, y.shape[1] * F, "power")
    return [b[:y.shape[1] * F].view(y.shape[1], F) for y, b in zip(Ys, bufs)]


def _raw_corr(Ys, Ws, taps, delay):
    """pk2_wpe_corr into poisoned buffers -> (R (B, F, D, D), P (B, F, D, C))"""
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    D = Cn * taps
    work, nbytes = _work(Ys, taps, delay)
    nR, nP = B * F * D * D * 2, B * F * D * Cn * 2
    Rm, Pm = _poisoned(nR), _poisoned(nP)
    _lib.check(_lib.lib().pk2_wpe_corr(_tab(Ys), _tab(Ws), _frames(Ys), B, Cn, F, taps, delay, _lib.ptr(work), nbytes,
                                       _lib.ptr(Rm), _lib.ptr(Pm), _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(Rm, nR, "R")
    _check_poison(Pm, nP, "P")
    _check_work(work, nbytes)
    return torch.view_as_complex(Rm[:nR].view(B, F, D, D, 2)), torch.view_as_complex(Pm[:nP].view(B, F, D, Cn, 2))


def _raw_solve(Rm, Pm, diag_load):
    """pk2_wpe_solve on (B, F, D, D) and (B, F, D, C) -> (G (B, F, D, C), nonfinite (B,))"""
    B, F, D, Cn = Pm.shape
    nG = B * F * D * Cn * 2
    G = _poisoned(nG)
    flag = torch.full((B + PAD,), -7, dtype=torch.int32, device="cuda")
    nbytes = (B * F * 4 + 255) // 256 * 256
    work = torch.full((nbytes // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().pk2_wpe_solve(_lib.ptr(Rm.contiguous()), _lib.ptr(Pm.contiguous()), B, Cn, F, D // Cn, diag_load,
                                        _lib.ptr(work), nbytes, _lib.ptr(G), _lib.ptr(flag), _lib.stream_ptr()))
    torch.cuda.synchronize()
    _check_poison(G, nG, "G")
    _check_work(work, nbytes)
    assert (flag[B:] == -7).all() and ((flag[:B] == 0) | (flag[:B] == 1)).all()
    return torch.view_as_complex(G[:nG].view(B, F, D, Cn, 2)), flag[:B]


def _raw_filter(Ys, G, delay, with_power=True):
    """pk2_wpe_filter with G (B, F, D, C) -> (list of X (C, N, F), list of power (N, F))"""
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    taps = G.shape[2] // Cn
    outs = [_poisoned(y.numel() * 2) for y in Ys]
    pows = [_poisoned(y.shape[1] * F) for y in Ys]
    _lib.check(_lib.lib().pk2_wpe_filter(_tab(Ys), _lib.ptr(G.contiguous()), _frames(Ys), B, Cn, F, taps, delay, _tab(outs),
                                         _tab(pows) if with_power else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for y, o, p in zip(Ys, outs, pows):
        _check_poison(o, y.numel() * 2, "X")
        if with_power:
            _check_poison(p, y.shape[1] * F, "power_out")
    return ([torch.view_as_complex(o[:y.numel() * 2].view(*y.shape, 2)) for y, o in zip(Ys, outs)],
            [p[:y.shape[1] * F].view(y.shape[1], F) for y, p in zip(Ys, pows)])


def _raw_wpe(Ys, taps, delay, iters, diag_load, nan_input=False):
    B, (Cn, _, F) = len(Ys), Ys[0].shape
    work, nbytes = _work(Ys, taps, delay)
    outs = [_poisoned(y.numel() * 2) for y in Ys]
    flag = torch.full((B + PAD,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().pk2_wpe(_tab(Ys), _frames(Ys), B, Cn, F, taps, delay, iters, diag_load, _lib.ptr(work), nbytes,
                                  _tab(outs), _lib.ptr(flag), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for y, o in zip(Ys, outs):
        if nan_input:       # the NaN of the input comes back: only the padding can be checked
            assert np.isnan(o[y.numel() * 2:].cpu().numpy()).all(), "X: the padding behind the result was written"
        else:
            _check_poison(o, y.numel() * 2, "X")
    _check_work(work, nbytes)
    assert (flag[B:] == -7).all()
    return [torch.view_as_complex(o[:y.numel() * 2].view(*y.shape, 2)) for y, o in zip(Ys, outs)], flag[:B]


def _rel(got, want):
    want = np.asarray(want)
    return float(np.abs(got.cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-300))


def _reference(Y, taps, delay, diag_load):
    lam = R.power(Y, np.float32)                       # the weight the correlation stage is given, exact in both
    Rm, Pm = R.correlations(Y, lam, taps, delay)
    G = R.solve(Rm, Pm, diag_load)[0].astype(np.complex64)
    return dict(Y=Y, taps=taps, delay=delay, diag_load=diag_load, power=R.power(Y), lam=lam, R=Rm, P=Pm, G=G,
                X=R.apply(Y, G, delay), full=R.wpe(Y, taps, delay, R.ITERATIONS, diag_load)[0])


@pytest.fixture(scope="module")
def want():
    """name -> the float64 restatement's results, computed once and left unchanged"""
    out = {}
    for name in R.CASES:
        _, taps, delay, _, _, dl, _, _ = R.CASES[name]
        out[name] = _reference(R.case_input(name), taps, delay, dl)
    for n, Y in zip(R.RAGGED["frames"], R.ragged_inputs()):
        out["ragged_%d" % n] = _reference(Y, R.RAGGED["taps"], R.RAGGED["delay"], R.RAGGED["diag_load"])
    return out


def _residual(Rm, Pm, G, diag_load):
    """max |R' G - P| in float64"""
    Rl = R.load(np.asarray(Rm).astype(np.complex128), diag_load)
    return float(np.abs(Rl @ np.asarray(G).astype(np.complex128) - np.asarray(Pm).astype(np.complex128)).max())


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_stage_matches_the_restatement(name, want):
    c = want[name]
    taps, delay, dl = c["taps"], c["delay"], c["diag_load"]
    Y = dev(c["Y"])
    Cn, N, F = Y.shape
    D = Cn * taps
    # power
    pw = _raw_power([Y])[0]
    err = _rel(pw, c["power"])
    print(name, "power rel err %.3e bound %.3e" % (err, POWER_TOL))
    assert err <= POWER_TOL
    assert _same(dereverb.wpe_power(Y), pw)
    # correlations, from the restatement's float32 weight
    lam = dev(c["lam"])
    Rm, Pm = _raw_corr([Y], [lam], taps, delay)
    assert tuple(Rm.shape) == (1, F, D, D) and tuple(Pm.shape) == (1, F, D, Cn)
    errR, errP = _rel(Rm[0], c["R"]), _rel(Pm[0], c["P"])
    print(name, "correlation rel err R %.3e P %.3e bound %.3e" % (errR, errP, CORR_TOL))
    assert errR <= CORR_TOL and errP <= CORR_TOL
    _assert_hermitian(Rm)
    if N <= delay:
        assert not Rm.any() and not Pm.any()
    Ra, Pa = dereverb.wpe_correlations(Y, lam, taps, delay)
    assert _same(Ra, Rm[0]) and _same(Pa, Pm[0])
    # the solve, on the device's own float32 R and P: its residual against that of the restatement's float64 G rounded once
    G, flag = _raw_solve(Rm, Pm, dl)
    assert flag.tolist() == [0]
    Rn, Pn = Rm[0].cpu().numpy(), Pm[0].cpu().numpy()
    ref_G, ref_bad = R.solve(Rn, Pn, dl)
    assert not ref_bad.any()
    res, ref_res = _residual(Rn, Pn, G[0].cpu().numpy(), dl), _residual(Rn, Pn, ref_G.astype(np.complex64), dl)
    print(name, "solve residual %.3e, the restatement's %.3e" % (res, ref_res))
    assert res <= 4 * ref_res
    assert _same(dereverb.wpe_filter_taps(Rm[0], Pm[0], dl), G[0]) and dereverb.last_nonfinite.tolist() == [0]
    # the filter and its power, with the restatement's G
    Gr = dev(c["G"][None])
    Xs, ps = _raw_filter([Y], Gr, delay)
    err = _rel(Xs[0], c["X"])
    print(name, "filter rel err %.3e bound %.3e" % (err, APPLY_TOL))
    assert err <= APPLY_TOL
    assert _same(ps[0], _raw_power([Xs[0].contiguous()])[0])
    assert _same(_raw_filter([Y], Gr, delay, with_power=False)[0][0], Xs[0])
    Xa, pa = dereverb.wpe_apply(Y, Gr[0], delay, with_power=True)
    assert _same(Xa, Xs[0]) and _same(pa, ps[0]) and _same(dereverb.wpe_apply(Y, Gr[0], delay), Xs[0])
    # the whole
    out, flag = _raw_wpe([Y], taps, delay, R.ITERATIONS, dl)
    err = _rel(out[0], c["full"])
    print(name, "wpe rel err %.3e bound %.3e" % (err, WPE_TOL))
    assert err <= WPE_TOL and flag.tolist() == [0]
    assert _same(dereverb.wpe(Y, taps, delay, R.ITERATIONS, dl), out[0]) and dereverb.last_nonfinite.tolist() == [0]
    if N <= delay:
        assert _same(out[0], Y)


@pytest.mark.parametrize("Cn,taps,delay,N,F", [(3, 4, 2, 200, 5), (8, 10, 3, 97, 3), (7, 10, 3, 33, 17), (2, 2, 1, 2 * R.P + 1, 3),
                                               (1, 1, 1, 5, 33), (5, 7, 3, R.P, 3)])
def test_exact_integer_correlations_bit_for_bit(Cn, taps, delay, N, F):
    Y, w = R.integer_input(Cn, N, F, seed=Cn * 100 + taps)
    wR, wP = R.correlations(Y, w, taps, delay)
    assert np.abs(wR).max() < 2 ** 24 and np.abs(wP).max() < 2 ** 24
    Rm, Pm = _raw_corr([dev(Y)], [dev(w)], taps, delay)
    assert np.array_equal(Rm[0].cpu().numpy(), wR.astype(np.complex64))
    assert np.array_equal(Pm[0].cpu().numpy(), wP.astype(np.complex64))
    _assert_hermitian(Rm)


def test_a_ragged_batch_equals_its_single_calls_bit_for_bit(want):
    r = R.RAGGED
    names = ["ragged_%d" % n for n in r["frames"]]
    taps, delay, dl = r["taps"], r["delay"], r["diag_load"]
    Ys = [dev(want[n]["Y"]) for n in names]
    assert [y.shape[1] for y in Ys] == list(r["frames"])
    pw, pw2 = _raw_power(Ys), _raw_power(Ys)
    Rm, Pm = _raw_corr(Ys, pw, taps, delay)
    R2, P2 = _raw_corr(Ys, pw, taps, delay)
    assert _same(Rm, R2) and _same(Pm, P2)
    G, flag = _raw_solve(Rm, Pm, dl)
    G2, _ = _raw_solve(Rm, Pm, dl)
    assert _same(G, G2) and flag.tolist() == [0] * 4
    Xs, ps = _raw_filter(Ys, G, delay)
    Xs2, ps2 = _raw_filter(Ys, G, delay)
    out, flag = _raw_wpe(Ys, taps, delay, R.ITERATIONS, dl)
    out2, _ = _raw_wpe(Ys, taps, delay, R.ITERATIONS, dl)
    assert flag.tolist() == [0] * 4
    api = dereverb.wpe(Ys, taps, delay, R.ITERATIONS, dl)
    for b, name in enumerate(names):
        one = [Ys[b]]
        assert _same(_raw_power(one)[0], pw[b]) and _same(pw[b], pw2[b]), name
        R1, P1 = _raw_corr(one, [pw[b]], taps, delay)
        assert _same(R1[0], Rm[b]) and _same(P1[0], Pm[b]), name
        G1, _ = _raw_solve(Rm[b:b + 1], Pm[b:b + 1], dl)
        assert _same(G1[0], G[b]), name
        X1, p1 = _raw_filter(one, G[b:b + 1], delay)
        assert _same(X1[0], Xs[b]) and _same(p1[0], ps[b]) and _same(Xs[b], Xs2[b]) and _same(ps[b], ps2[b]), name
        assert _same(_raw_wpe(one, taps, delay, R.ITERATIONS, dl)[0][0], out[b]) and _same(out[b], out2[b]), name
        assert _same(api[b], out[b]) and _same(dereverb.wpe(Ys[b], taps, delay, R.ITERATIONS, dl), out[b]), name
        # and against the restatement
        c = want[name]
        assert _rel(Rm[b], R.correlations(c["Y"], pw[b].cpu().numpy(), taps, delay)[0]) <= CORR_TOL, name
        assert _rel(out[b], c["full"]) <= WPE_TOL, name
    # the list forms of the stage functions make the same bits
    assert all(_same(a, b) for a, b in zip(dereverb.wpe_power(Ys), pw))
    Ra, Pa = dereverb.wpe_correlations(Ys, pw, taps, delay)
    assert all(_same(a, b) for a, b in zip(Ra, Rm)) and all(_same(a, b) for a, b in zip(Pa, Pm))
    Ga = dereverb.wpe_filter_taps(Ra, Pa, dl)
    assert all(_same(a, b) for a, b in zip(Ga, G))
    assert all(_same(a, b) for a, b in zip(dereverb.wpe_apply(Ys, Ga, delay), Xs))


def test_more_utterances_than_one_launch_takes():
    """35 utterances are two launches per stage (32 + 3): the second group's tables, workspace and outputs are its own"""
    frames = [5 + (7 * b) % 23 for b in range(35)]
    Ys = [dev(R.make_input(2, n, 5, 1, 100 + b)) for b, n in enumerate(frames)]
    out, flag = _raw_wpe(Ys, 3, 1, 2, 1e-3)
    assert flag.tolist() == [0] * 35
    pw = _raw_power(Ys)
    Rm, Pm = _raw_corr(Ys, pw, 3, 1)
    G, _ = _raw_solve(Rm, Pm, 1e-3)
    Xs, ps = _raw_filter(Ys, G, 1)
    for b in (0, 31, 32, 34):
        one = [Ys[b]]
        assert _same(_raw_wpe(one, 3, 1, 2, 1e-3)[0][0], out[b]), b
        assert _same(_raw_power(one)[0], pw[b]), b
        R1, P1 = _raw_corr(one, [pw[b]], 3, 1)
        assert _same(R1[0], Rm[b]) and _same(P1[0], Pm[b]), b
        X1, p1 = _raw_filter(one, G[b:b + 1], 1)
        assert _same(X1[0], Xs[b]) and _same(p1[0], ps[b]), b


def test_a_non_finite_bin_passes_through_and_raises_the_flag(want):
    c = want["c3_k2_d1_n97_f33_zero"]
    taps, delay, dl = c["taps"], c["delay"], c["diag_load"]
    Rn, Pn = c["R"].astype(np.complex64), c["P"].astype(np.complex64)
    bad_R, bad_P = Rn.copy(), Pn.copy()
    bad_R[4, 1, 2] = np.nan
    bad_P[20, 0, 0] = np.inf
    G, flag = _raw_solve(dev(np.stack([Rn, bad_R, Rn])), dev(np.stack([Pn, Pn, bad_P])), dl)
    assert flag.tolist() == [0, 1, 1]
    G = G.cpu().numpy()
    assert not G[1, 4].any() and not G[2, 20].any() and np.isfinite(G).all()
    keep = np.ones(Rn.shape[0], bool)
    keep[4] = False
    assert np.array_equal(G[1, keep], G[0, keep]) and G[0, 4].any()
    # a matrix that is not positive definite is refused the same way
    neg = Rn.copy()
    neg[7] = -neg[7]
    Gn, flag = _raw_solve(dev(neg[None]), dev(Pn[None]), dl)
    Gn = Gn.cpu().numpy()
    keep[:] = True
    keep[7] = False
    assert flag.tolist() == [1] and not Gn[0, 7].any() and np.array_equal(Gn[0, keep], G[0, keep])
    # the whole: a NaN in one bin leaves that bin as it was, bit for bit, and the other bins what they are without it
    Y = c["Y"].copy()
    clean, flag = _raw_wpe([dev(Y)], taps, delay, 2, dl)
    assert flag.tolist() == [0]
    Y[1, 50, 4] = np.nan
    out, flag = _raw_wpe([dev(Y), dev(c["Y"])], taps, delay, 2, dl, nan_input=True)
    assert np.isnan(out[0].cpu().numpy()).sum() == 1
    assert flag.tolist() == [1, 0]
    assert _same(out[0][:, :, 4].contiguous(), dev(Y)[:, :, 4].contiguous())
    others = [f for f in range(Y.shape[2]) if f != 4]
    assert _same(out[0][:, :, others].contiguous(), clean[0][:, :, others].contiguous()) and _same(out[1], clean[0])


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
CFG = dict(fft_size=64, frame_len=50, frame_shift=20)


def _array_signal(n=6000, n_mics=4):
    """(n_mics, n) on the device: a synthetic utterance in a sampled room, made by rirgen and the simulator"""
    from pykaldi2_amd import beamform, rirgen, synth
    np.random.seed(5)
    x = _lib.h2d(synth.waveform(np.random.default_rng(3), n / 16000.0)[:n], DEV)
    room, t60, mic, src = rirgen.sample_online_room((0.4, 0.6), 1, mic_positions=beamform.array_geometry(n_mics, 0.05))
    b = rirgen.rirgen_batch([dict(room=room, source_loc=src, mic_loc=mic, t60=t60)], device=DEV)
    mixed, _ = simulation.SimpleSimulator(use_rir=True, use_noise=False)(x, None, b.rirs[0][0], None, normalize_gain=True,
                                                                         rir_delays=[b.delays[0][0]])
    return mixed.contiguous()


def test_dereverberator_in_the_time_domain():
    wav = _array_signal()
    n = wav.shape[1]
    drv = dereverb.Dereverberator(simulation.SpectrumAnalyzer(config=dict(CFG, do_dither=True)), taps=5, delay=2, iterations=2)
    got = drv(wav)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (4, n) and torch.isfinite(got).all()
    assert drv.last_nonfinite.tolist() == [0]
    spec = drv.analyze(wav)
    assert tuple(spec.shape) == (4, drv.analyzer.num_frames(n), 33)
    X = drv.spectrum(spec)
    assert _same(drv.analyzer.synthesize(X)[:, :n], got)
    # against the restatement on the downloaded spectrum; the bound is 4 x the restatement's own float32-mode error there
    Y = spec.cpu().numpy()
    full = R.wpe(Y, 5, 2, 2, 1e-3)[0]
    own = np.abs(R.wpe(Y, 5, 2, 2, 1e-3, np.float32)[0] - full).max() / np.abs(full).max()
    err = _rel(X, full)
    print("Dereverberator: spectrum rel err %.3e, the float32 mode's %.3e" % (err, own))
    assert own < 1e-3 and err <= 4 * own
    assert float((got - wav).abs().max()) > 1e-3 * float(wav.abs().max())          # it does something
    # one channel, 1-D in and out; the batch form gives the single calls' bits
    one = drv(wav[0].contiguous())
    assert tuple(one.shape) == (n,) and torch.isfinite(one).all()
    short = wav[:, :n - 173].contiguous()
    outs = drv.batch([wav, short])
    assert _same(outs[0], got) and _same(outs[1], drv(short)) and tuple(outs[1].shape) == (4, n - 173)


def test_the_scene_loses_its_late_reverberation_on_the_device():
    Y, E = R.scene(4, 600, 9, 3, seed=0)
    want = R.reduction_db(R.wpe(Y.astype(np.complex64), 10, 3, 3, 1e-3)[0], Y, E)
    got = dereverb.wpe(dev(Y.astype(np.complex64)), 10, 3, 3, 1e-3)
    have = R.reduction_db(got.cpu().numpy().astype(np.complex128), Y, E)
    print("late reverberation: -%.2f dB on the device, -%.2f dB in the restatement" % (have, want))
    assert want >= 3.0 and abs(have - want) <= 0.1 and dereverb.last_nonfinite.tolist() == [0]


def _pool(**extra):
    from pykaldi2_amd import data
    dc = dict(online_rir=True, use_reverb=True, use_dir_noise=True, simulation_prob=1.0, gain_norm=True)
    dc.update(extra)
    return data.SimulationPool.from_config({"synthetic": True, "data_config": dc})


def _utterance():
    from pykaldi2_amd import synth
    return synth.waveform(np.random.default_rng(3), 1.3)


def _state_after(pool, x, seed):
    np.random.seed(seed)
    y = pool.maybe_simulate(x, DEV)
    return y, np.random.get_state()[1].copy()


def test_simulation_pool_with_the_key_alone():
    x = _utterance()
    plain, state0 = _state_after(_pool(), x, 11)
    pool = _pool(wpe={"taps": 8})
    y, state = _state_after(pool, x, 11)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0],) and torch.isfinite(y).all()
    assert np.array_equal(state, state0)                       # the key adds no draw
    assert _same(y, _state_after(pool, x, 11)[0])
    assert _same(y, pool.dereverb(plain)) and not _same(y, plain)      # the single-channel simulation, dereverberated with C = 1
    # shorter than one analysis frame: as it is
    tiny = x[:300]
    assert _same(_state_after(pool, tiny, 12)[0], _state_after(_pool(), tiny, 12)[0])


def test_simulation_pool_with_the_key_and_the_beamformer():
    from pykaldi2_amd import beamform
    x = _utterance()
    bf_only, state0 = _state_after(_pool(beamform={"n_mics": 4}), x, 11)
    pool = _pool(beamform={"n_mics": 4}, wpe=True)
    y, state = _state_after(pool, x, 11)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0],) and torch.isfinite(y).all()
    assert y.abs().max() > 0 and np.array_equal(state, state0) and not _same(y, bf_only)
    assert _same(y, _state_after(pool, x, 11)[0])
    assert pool.dereverb.last_nonfinite.tolist() == [0] and beamform.last_nonfinite.tolist() == [0]


def test_simulation_pool_without_the_key_is_the_unchanged_path():
    """maybe_simulate without the key against the single-channel steps written out as they were before the key existed"""
    pool, x = _pool(), _utterance()
    assert pool.wpe is None and pool.beamform is None
    np.random.seed(12)
    got = pool.maybe_simulate(x, DEV)
    state = np.random.get_state()[1].copy()
    np.random.seed(12)
    xd = _lib.h2d(x, DEV)
    assert not np.random.random() > pool.prob
    noise = pool._on_device("n", int(np.random.choice(len(pool.noises))), DEV)[0]
    src_rir, noise_rir, delays = pool.online_rirs(2, DEV)
    want, _ = pool.sim(xd, [noise], src_rir, [noise_rir], normalize_gain=pool.gain_norm, rir_delays=delays)
    assert _same(got, want) and tuple(got.shape) == (x.shape[0],)
    assert np.array_equal(np.random.get_state()[1], state)


def test_argument_errors():
    Y = torch.zeros(3, 5, 17, dtype=torch.complex64, device="cuda")
    lam = torch.ones(5, 17, device="cuda")
    G = torch.zeros(17, 6, 3, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="complex64"):
        dereverb.wpe(torch.view_as_real(Y))
    with pytest.raises(ValueError, match="CUDA"):
        dereverb.wpe(Y.cpu())
    with pytest.raises(ValueError, match="at most 8"):
        dereverb.wpe(torch.zeros(9, 5, 17, dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="order 81"):
        dereverb.wpe(Y, taps=27)
    for kw, word in ((dict(delay=0), "delay"), (dict(delay=9), "delay"), (dict(iterations=0), "iterations"),
                     (dict(iterations=9), "iterations"), (dict(taps=0), "taps"), (dict(diag_load=-1), "diag_load")):
        with pytest.raises(ValueError, match=word):
            dereverb.wpe(Y, **kw)
    with pytest.raises(ValueError, match="first one"):
        dereverb.wpe([Y, Y[:2].contiguous()])
    with pytest.raises(ValueError, match=r"\(N, F\) = \(5, 17\)"):
        dereverb.wpe_correlations(Y, torch.ones(4, 17, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        dereverb.wpe_correlations(Y, lam.double())
    with pytest.raises(ValueError, match=r"\(F, D, C\)"):
        dereverb.wpe_apply(Y, G[:, :, :2].contiguous())
    with pytest.raises(ValueError, match=r"\(F, D, D\)"):
        dereverb.wpe_filter_taps(torch.zeros(17, 6, 5, dtype=torch.complex64, device="cuda"), G)
    drv = dereverb.Dereverberator(simulation.SpectrumAnalyzer(config=CFG))
    with pytest.raises(ValueError, match="at most 8"):
        drv(torch.zeros(9, 400, device="cuda"))
    with pytest.raises(ValueError, match="order 90"):
        dereverb.Dereverberator(drv.analyzer, taps=30)(torch.zeros(3, 400, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        drv(torch.zeros(3, 400, dtype=torch.float64, device="cuda"))
