"""STFT, inverse STFT, the 'count' clean mask's cutoff, the ideal masks and the simulators' gen_mask on the device, against
the float64 restatement tests/mask_ref.py (which tests/test_mask_host.py pins to the reference's own outputs).  Spectra
and masks are frame-major (N, F)."""
import numpy as np
import pytest

import mask_ref as R

pytestmark = pytest.mark.gpu

# float32 kernels against float64 references.  The rule: run the restatement once in float32 on the CPU
# against the float64 result and take 4 x its largest error relative to max|want|.  Measured with mask_ref (numpy's
# float32 transform), never with the device:
STFT_TOL = 4 * 5.04e-8       # mask_ref.stft(float32) over the eight cases below: 3.52e-8 .. 5.04e-8
ISTFT_TOL = {"d6000": 4 * 2.57e-7, "hann64": 4 * 9.28e-6}     # istft(stft(x)) in float32, samples with a window sum >= 1e-3 max
SOFT_TOL = 4 * 5.97e-7       # the soft mask (max 1) in float32 over the five mask cases: 2.98e-7 .. 5.96e-7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stft_case(name):
    if name.startswith("d"):
        n = int(name[1:])
        return R.DEFAULT, R.inputs(1 if n == 6000 else 4 if n == 3055 else 3, n, 5)[0]
    cfg, n, seed = R.STFT_CASES[name]
    return cfg, R.inputs(seed, n, 5)[0]


def _analyzer(cfg, **kw):
    from pykaldi2_amd import simulation
    return simulation.SpectrumAnalyzer(config=dict(cfg, **kw))


@pytest.fixture(scope="module")
def mask_cases():
    """name -> (clean, distorted, dither (2, n) float32, float64 restatement with that dither); computed once"""
    out = {}
    for name, case in R.MASK_CASES.items():
        c, d = R.inputs(*case)
        dith = (1e-5 * np.random.RandomState(100 + case[0]).standard_normal((2, case[1]))).astype(np.float32)
        out[name] = (c, d, dith, R.mask(c, d, dither=dith))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward STFT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d6000", "d400", "d401", "d3055", "hann64", "bartlett32", "hamming1024", "hamming4096"])
def test_gpu_stft_matches_restatement(name):
    """default configuration at 36 padded frames, one frame, a second frame that is almost all padding, an odd length; then
    fft 64 (256 frames' worth of LDS cut to 16 per workgroup), fft 32 with an odd shift (unaligned spans), 1024 and 4096
    (two frames per workgroup)"""
    import torch
    cfg, x = _stft_case(name)
    an = _analyzer(cfg, do_dither=False)
    got = an.analyze(dev(x))
    want = R.stft(x, **cfg)
    assert got.dtype == torch.complex64 and tuple(got.shape) == want.shape == (an.num_frames(len(x)), an.n_bin)
    err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(name, "stft rel err %.3e bound %.3e" % (err, STFT_TOL))
    assert err <= STFT_TOL
    assert not torch.view_as_real(got)[:, 0, 1].any() and not torch.view_as_real(got)[:, -1, 1].any()    # DC, Nyquist real


def test_gpu_stft_batch_dither_and_errors():
    import torch
    from pykaldi2_amd import _lib, simulation
    cfg = R.DEFAULT
    n = 3055
    x = np.stack([R.inputs(s, n, 5)[0] for s in (4, 8, 9)])
    dith = (1e-5 * np.random.RandomState(3).standard_normal((3, n))).astype(np.float32)
    an, quiet = _analyzer(cfg), _analyzer(cfg, do_dither=False)
    dx, dd = dev(x), dev(dith)
    # explicit dither: against the restatement fed the same array; a 3-row batch equals the single-row calls bit for bit
    batch = an.analyze(dx, dither=dd)
    for r in range(3):
        want = R.stft(x[r], dither=dith[r], **cfg)
        err = np.abs(batch[r].cpu().numpy() - want).max() / np.abs(want).max()
        print("row", r, "explicit dither rel err %.3e bound %.3e" % (err, STFT_TOL))
        assert err <= STFT_TOL
        assert torch.equal(torch.view_as_real(an.analyze(dx[r], dither=dd[r])), torch.view_as_real(batch[r]))
    nod = quiet.analyze(dx)
    assert not torch.equal(torch.view_as_real(nod), torch.view_as_real(batch))
    for r in range(3):
        assert torch.equal(torch.view_as_real(quiet.analyze(dx[r])), torch.view_as_real(nod[r]))
    # the generator path is the explicit path fed 1e-5 * its draws, bit for bit -- odd n, and an odd shift whose spans begin
    # inside a sample pair; two seeded runs are bit-equal; another seed, and no seed, differ
    for c, sig in ((cfg, dx), (R.STFT_CASES["bartlett32"][0], dx[:, :333].contiguous())):
        a = _analyzer(c)
        m = sig.shape[1]
        z = simulation.iso_gauss(17, 3, (m + 1) // 2).view(3, -1)[:, :m]
        explicit = (z * torch.tensor(1e-5, dtype=torch.float32, device="cuda")).contiguous()
        got = a.analyze(sig, seed=17)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(a.analyze(sig, dither=explicit)))
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(a.analyze(sig, seed=17)))
        assert not torch.equal(torch.view_as_real(got), torch.view_as_real(a.analyze(sig, seed=18)))
    np.random.seed(5)
    g1 = an.analyze(dx)
    np.random.seed(5)
    assert torch.equal(torch.view_as_real(g1), torch.view_as_real(an.analyze(dx)))      # seed=None: one numpy draw per call
    np.random.seed(5)
    assert torch.equal(torch.view_as_real(g1), torch.view_as_real(an.analyze(dx, seed=int(np.random.randint(0, 2 ** 31 - 1)))))
    # more rows than one launch's table holds
    many = dev(np.stack([np.roll(x[0], 7 * i) for i in range(19)]))
    got = quiet.analyze(many)
    assert torch.equal(torch.view_as_real(got[18]), torch.view_as_real(quiet.analyze(many[18])))
    # errors: a signal shorter than one frame, parameters out of range (Python and the library itself)
    with pytest.raises(ValueError):
        quiet.analyze(dx[0, :399].contiguous())
    with pytest.raises((ValueError, _lib.Pk2Error)):
        _analyzer(dict(cfg, fft_size=500), do_dither=False).analyze(dx[0])
    L, w, out = _lib.lib(), dev(np.hamming(400).astype(np.float32)), torch.zeros(18, 257, 2, device="cuda")
    tab = (_lib.C.c_void_p * 1)(dx[0].data_ptr())
    for fft, ln, sh, m in ((8192, 400, 160, n), (512, 513, 160, n), (512, 400, 401, n), (512, 400, 0, n), (512, 400, 160, 399)):
        assert L.pk2_stft_f32(tab, 1, m, fft, ln, sh, _lib.ptr(w), None, 0, 0, _lib.ptr(out), _lib.stream_ptr()) != 0
    assert L.pk2_stft_num_frames(399, 400, 160) == -1 and L.pk2_stft_num_frames(401, 400, 160) == 2


# ---------------------------------------------------------------------------------------------------------------------
# 2. inverse STFT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d6000", "hann64"])
def test_gpu_istft_matches_restatement_and_signal(name):
    import torch
    cfg, x = _stft_case(name)
    an = _analyzer(cfg, do_dither=False)
    spec = an.analyze(dev(x))
    got = an.synthesize(spec)
    want, ws = R.istft(R.stft(x, **cfg), **cfg)
    N = spec.shape[0]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (cfg["fft_size"] + cfg["frame_shift"] * (N - 1),)
    got = got.cpu().numpy()
    # hann: the first and last few samples have a window sum near zero and are left out (the tail beyond the last frame's
    # frame_len taps, where nothing is divided, is checked below)
    ok = ws >= 1e-3 * ws.max()
    assert 1 - ok.mean() <= 0.02
    tol = ISTFT_TOL[name]
    err = np.abs(got - want)[ok].max() / np.abs(want[ok]).max()
    errx = np.abs(got[:len(x)] - x)[ok[:len(x)]].max() / np.abs(x).max()
    print(name, "istft rel err %.3e against x %.3e bound %.3e, left out %.2f %%" % (err, errx, tol, 100 * (1 - ok.mean())))
    assert err <= tol and errx <= tol
    tail = ws <= 1e-10
    if tail.any():          # the unnormalised tail: the frames' transforms beyond the window, zero up to rounding
        assert np.abs(got - want)[tail].max() <= tol * np.abs(want[ok]).max()
    # a batch equals the single calls bit for bit
    both = an.synthesize(torch.stack([spec, spec.flip(0)]))
    assert np.array_equal(both[0].cpu().numpy(), got) and torch.equal(both[1], an.synthesize(spec.flip(0).contiguous()))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the 'count' clean mask's cutoff alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.THRESHOLD_NAMES)
def test_gpu_count_threshold_equals_sort_and_cumsum(name):
    from pykaldi2_amd import simulation
    p, thr = R.threshold_arrays()[name]
    want = R.count_mask(p.astype(np.float64), thr)
    v, strict, vstar = simulation.mask_count_threshold(dev(p), thr).cpu().numpy().tolist()
    assert np.array_equal(R.decide(p, np.float32(v), bool(strict)), want)
    mv, mstrict = R.descent_threshold(p, thr)                      # the host model of the descent, bit for bit
    assert (np.float32(v), bool(strict)) == (mv, mstrict)
    wv, ok = R.count_threshold(p.astype(np.float64), thr)
    assert vstar == (wv if ok else 0.0)                             # the reference's cutoff itself (0: nothing lies below v)
    if name in ("one", "two_degenerate"):
        assert want.all() and not ok
    if name == "equal1000":
        assert not want.any()


def test_gpu_count_threshold_batch_equals_single_calls():
    import torch
    from pykaldi2_amd import simulation
    rs = np.random.RandomState(6)
    p = dev(rs.randint(0, 5000, size=(3, 257 * 36)).astype(np.float32) * np.array([[1.0], [64.0], [0.125]], np.float32))
    got = simulation.mask_count_threshold(p)
    assert got.shape == (3, 3)
    for s in range(3):
        assert torch.equal(got[s], simulation.mask_count_threshold(p[s]))
    assert torch.equal(got, simulation.mask_count_threshold(p))      # and twice the same bits (atomics in any order)


# ---------------------------------------------------------------------------------------------------------------------
# 4. masks
# ---------------------------------------------------------------------------------------------------------------------
def _estimator(**kw):
    from pykaldi2_amd import simulation
    return simulation.MaskEstimator(simulation.SpectrumAnalyzer(), **kw)


@pytest.mark.parametrize("name", sorted(R.MASK_CASES))
def test_gpu_binary_mask_equals_restatement(mask_cases, name):
    """Every bin equal, except the decision-edge ones: |snr - 0.5| <= 0.01 dB or |P_c / v* - 1| <= 1e-3 in the float64
    restatement (0.01-0.06 % of the bins on these inputs; a float32 run of the restatement flips no bin outside them)."""
    c, d, dith, want = mask_cases[name]
    est = _estimator()
    got = est.get_mask_from_parallel_data(dev(c), dev(d), dither=dev(dith))
    assert tuple(got.shape) == want["mask"].shape
    got = got.cpu().numpy()
    edge = (np.abs(want["snr_db"] - 0.5) <= 0.01) | (np.abs(want["power_clean"] / want["v"] - 1) <= 1e-3)
    f32 = R.mask(c, d, dither=dith, dtype=np.float32)["mask"]
    print(name, "decision-edge share %.3f %%, float32 restatement flips outside it: %d, device flips inside it: %d"
          % (100 * edge.mean(), int(((f32 != want["mask"]) & ~edge).sum()), int(((got != want["mask"]) & edge).sum())))
    assert edge.mean() <= 0.005 and not ((f32 != want["mask"]) & ~edge).any()
    assert np.array_equal(got[~edge], want["mask"][~edge])
    assert set(np.unique(got)) <= {0.0, 1.0}
    v, strict, vstar = est.last_threshold[0].cpu().numpy().tolist()
    print(name, "cutoff: device %.6e (v %.6e, strict %d) restatement %.6e" % (vstar, v, strict, want["v"]))
    assert abs(vstar / want["v"] - 1) <= 1e-3


def test_gpu_soft_mask_vad_batch_and_silence(mask_cases):
    import torch
    from pykaldi2_amd import simulation
    c, d, dith, want = mask_cases["m1"]
    est = _estimator()
    dc, dd, ddi = dev(c), dev(d), dev(dith)
    # soft mask, outside the clean mask's edge
    got = est.get_mask_from_parallel_data(dc, dd, use_soft_mask=True, dither=ddi).cpu().numpy()
    soft = R.mask(c, d, dither=dith, use_soft_mask=True)["mask"]
    cedge = np.abs(want["power_clean"] / want["v"] - 1) <= 1e-3
    err = np.abs(got - soft)[~cedge].max()
    print("soft mask err %.3e bound %.3e, max %.3f" % (err, SOFT_TOL, soft.max()))
    assert err <= SOFT_TOL and got.max() <= 1.0 and 0 < (got > 0).mean() < 0.2
    # vad per frame: frames at or below 0.5 are zeroed, the others untouched
    binary = est.get_mask_from_parallel_data(dc, dd, dither=ddi)
    vad = np.linspace(0.0, 1.0, binary.shape[0]).astype(np.float32)
    vad[20] = 0.5           # (0.57 before: the comparison is strict)
    with_vad = est.get_mask_from_parallel_data(dc, dd, vad=vad, dither=ddi)
    keep = torch.from_numpy(vad > 0.5).cuda()
    assert torch.equal(with_vad[keep], binary[keep]) and not with_vad[~keep].any() and binary[~keep].any()
    assert torch.equal(with_vad, est.get_mask_from_parallel_data(dc, dd, vad=dev(vad), dither=ddi))
    # three sources against one mixture: equal to the three single calls bit for bit (the dither rows passed along)
    rs = np.random.RandomState(9)
    srcs = np.stack([c, R.inputs(8, 6000, 5)[0], R.inputs(9, 6000, 5)[0]])
    dith4 = (1e-5 * rs.standard_normal((4, 6000))).astype(np.float32)
    ds, dd4 = dev(srcs), dev(dith4)
    batch = est.get_mask_from_parallel_data(ds, dd, dither=dd4)
    thr = est.last_threshold.clone()
    assert tuple(batch.shape) == (3,) + want["mask"].shape and thr.shape == (3, 3)
    assert torch.equal(batch, est.get_mask_from_parallel_data(list(ds.unbind(0)), dd, dither=dd4))
    for s in range(3):
        one = est.get_mask_from_parallel_data(ds[s], dd, dither=dd4[[s, 3]].contiguous())
        assert torch.equal(one, batch[s]) and torch.equal(est.last_threshold[0], thr[s])
    assert len({float(batch[s].sum()) for s in range(3)}) == 3
    # the generator's dither: seeded runs are bit-equal, and the clean and the distorted signal get different rows
    a = est.get_mask_from_parallel_data(ds, dd, seed=3)
    assert torch.equal(a, est.get_mask_from_parallel_data(ds, dd, seed=3))
    twice = simulation.SpectrumAnalyzer().analyze(torch.stack([dd, dd]), seed=3)
    assert not torch.equal(torch.view_as_real(twice[0]), torch.view_as_real(twice[1]))
    # an all-zero clean signal without dither: all zeros, no NaN; other clean mask types: all ones, 'floor' is not built
    quiet = simulation.MaskEstimator(simulation.SpectrumAnalyzer(do_dither=False))
    z = quiet.get_mask_from_parallel_data(torch.zeros_like(dc), dd)
    assert not torch.isnan(z).any() and not z.any()
    plain = simulation.MaskEstimator(simulation.SpectrumAnalyzer(), clean_mask_type="none")
    assert plain.get_mask_from_parallel_data(dc, dd, dither=ddi).sum() > binary.sum() and plain.last_threshold is None
    with pytest.raises(NotImplementedError):
        simulation.MaskEstimator(simulation.SpectrumAnalyzer(), clean_mask_type="floor").get_mask_from_parallel_data(dc, dd)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the simulators' gen_mask
# ---------------------------------------------------------------------------------------------------------------------
def _utterance():
    rs = np.random.RandomState(71)
    wavs = [R.inputs(21, 4000, 5)[0], R.inputs(22, 3000, 5)[0]]
    rirs = []
    for d in (5, 9, 3):
        r = 0.3 * rs.standard_normal((2, 300)) * np.exp(-np.arange(300) / 60.0)[None, :]
        r[:, :d] = 0
        r[0, d], r[1, d + 1] = 1.0, 0.9
        rirs.append(r.astype(np.float32))
    noise = (0.05 * rs.standard_normal(5000)).astype(np.float32)
    return wavs, rirs[:2], [noise], rirs[2:]


def test_gpu_multi_source_simulator_gen_mask():
    import torch
    from pykaldi2_amd import simulation
    wavs, rirs, noises, noise_rirs = _utterance()
    args = lambda: ([dev(w) for w in wavs], [dev(x) for x in noises], [dev(r) for r in rirs], [dev(r) for r in noise_rirs])
    sim = simulation.MultiSourceSimulator(mask_estimator=simulation.MaskEstimator(simulation.SpectrumAnalyzer()))
    with pytest.raises(NotImplementedError):        # a simulator built without an estimator cannot make masks
        simulation.MultiSourceSimulator()(*args(), gen_mask=True)
    np.random.seed(81)
    mixed, early, masks, cfg = sim(*args(), gen_mask=True, normalize_gain=False, mask_seed=5)
    assert mixed.shape == (2, 4000) and len(early) == 2 and len(masks) == 2 and "mask" not in cfg
    N = simulation.stft_num_frames(4000, 400, 160)
    assert all(tuple(m.shape) == (N, 257) and m.dtype == torch.float32 for m in masks)
    # the masks are MaskEstimator's on channel 0 of the returned early reverberation against channel 0 of the mixture
    est = simulation.MaskEstimator(simulation.SpectrumAnalyzer())
    want = est.get_mask_from_parallel_data([e[0] for e in early], mixed[0], seed=5)
    assert torch.equal(torch.stack(masks), want)
    assert all(0 < float(m.mean()) < 0.5 for m in masks) and not torch.equal(masks[0], masks[1])
    # everything else is the gen_mask=False, get_early_reverb=True run under the same numpy seed, bit for bit
    np.random.seed(81)
    mixed0, early0, none, cfg0 = sim(*args(), gen_mask=False, normalize_gain=False, get_early_reverb=True)
    assert none is None and torch.equal(mixed, mixed0) and all(torch.equal(a, b) for a, b in zip(early, early0))
    assert sorted(cfg) == sorted(cfg0)
    for k in cfg:
        if isinstance(cfg[k], torch.Tensor):
            # `scale` is a float64 diagnostic whose power sums the mixer's kernel adds up with double atomics: its last
            # bits differ between two runs of the very same call, with or without gen_mask.  What the kernels apply is
            # its float32 rounding (the mixtures above are bit-equal).
            assert torch.equal(cfg[k].float(), cfg0[k].float()) and float(((cfg[k] - cfg0[k]) / cfg0[k]).abs().max()) <= 1e-12, k
        else:
            assert np.array_equal(np.asarray(cfg[k]), np.asarray(cfg0[k])), k
    # with the gain normalisation the masks are the same ones (they are made before it)
    np.random.seed(81)
    mixed1, early1, masks1, cfg1 = sim(*args(), gen_mask=True, normalize_gain=True, mask_seed=5)
    assert torch.equal(torch.stack(masks1), want) and "gain_norm_scale" in cfg1 and not torch.equal(mixed1, mixed)
    # no mask_seed: one more numpy draw, after all the others
    np.random.seed(81)
    sim(*args(), gen_mask=False, normalize_gain=False)
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    np.random.seed(81)
    masks2 = sim(*args(), gen_mask=True, normalize_gain=False)[2]
    assert torch.equal(torch.stack(masks2), est.get_mask_from_parallel_data([e[0] for e in early], mixed[0], seed=seed))


def test_gpu_simple_simulator_gen_mask():
    import torch
    from pykaldi2_amd import simulation
    wavs, rirs, noises, noise_rirs = _utterance()
    est = simulation.MaskEstimator(simulation.SpectrumAnalyzer())
    sim = simulation.SimpleSimulator(mask_estimator=est)
    with pytest.raises(NotImplementedError):
        simulation.SimpleSimulator()(dev(wavs[0]), gen_mask=True)
    # 1-D inputs come back 1-D
    np.random.seed(82)
    mixed, early, masks, cfg = sim(dev(wavs[0]), [dev(noises[0])], dev(rirs[0][0]), [dev(noise_rirs[0][0])], normalize_gain=False,
                                   gen_mask=True, mask_seed=6)
    assert mixed.shape == (4000,) and len(early) == 1 and early[0].shape == (4000,) and len(masks) == 1
    assert torch.equal(masks[0], est.get_mask_from_parallel_data(early[0], mixed, seed=6)) and 0 < float(masks[0].mean()) < 0.5
    np.random.seed(82)
    mixed0, cfg0 = sim(dev(wavs[0]), [dev(noises[0])], dev(rirs[0][0]), [dev(noise_rirs[0][0])], normalize_gain=False)
    assert np.abs((mixed - mixed0).cpu().numpy()).max() <= 1e-5 * float(mixed0.abs().max())     # (the batched kernel's sums)
    assert np.array_equal(cfg["dir_snr"], cfg0["dir_snr"]) and cfg["dir_start"] == cfg0["dir_start"]
    # multi-channel RIRs; and without RIRs the clean side is the source itself
    np.random.seed(82)
    mixed, early, masks, cfg = sim(dev(wavs[0]), [dev(noises[0])], dev(rirs[0]), [dev(noise_rirs[0])], gen_mask=True, mask_seed=6)
    assert mixed.shape == (2, 4000) and early[0].shape == (2, 4000) and masks[0].shape == (24, 257)
    np.random.seed(82)
    mixed, early, masks, cfg = sim(dev(wavs[0]), [dev(noises[0])], normalize_gain=False, gen_mask=True, mask_seed=6)
    assert torch.equal(early[0], dev(wavs[0])) and torch.equal(masks[0], est.get_mask_from_parallel_data(dev(wavs[0]), mixed, seed=6))
