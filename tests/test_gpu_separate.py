"""pykaldi2_amd.separate on the device against the float64 restatement tests/perm_align_ref.py: the aligner on identical
float32 inputs with poisoned buffers and checked padding, batch independence and run-to-run identity bit for bit, the whole
blind chain (random start, EM, alignment, noise last) on two scenes, the per-speaker MVDR, the command line, and the
existing front-end kinds left as they were."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perm_align_ref as R  # noqa: E402

from pykaldi2_amd import _lib, cgmm, separate  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The rule: the restatement's float32 mode on the CPU against its float64 result over these very cases, 4 x
# the largest error.  Measured with `python tests/perm_align_ref.py`, never with the device:
MARGIN_TOL = 4 * 2.22e-6      # margin over R.GPU_KS x R.GPU_FS x R.GPU_NS: 0 (one frame) .. 2.22e-6
BLIND_MASK_TOL = 4 * 1.49e-4  # aligned masks of the two blind scenes after 20 iterations (absolute): 5.66e-5, 1.49e-4
PAD = 64                      # poisoned elements behind every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _tab(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _poisoned(count):
    return torch.full((count + PAD,), float("nan"), dtype=torch.float32, device="cuda")


def _taken(buf, count, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[count:]).all(), "%s: the padding behind the result was written" % what
    assert not np.isnan(got[:count]).any(), "%s: an element of the result was not written" % what
    return got[:count]


def _raw_align(lams, Rm=None, la=None, refine=3, noise_last=True):
    """pk2_perm_align into poisoned buffers with a poisoned workspace -> (masks [(K, N, F)], R, la, perm (B, F, K),
    margin (B, F)) as numpy"""
    B, (K, _, F) = len(lams), lams[0].shape
    frames = (C.c_int32 * B)(*[x.shape[1] for x in lams])
    nbytes = _lib.lib().pk2_perm_align_workspace_bytes(frames, B, F, K)
    assert nbytes > 0 and nbytes % 4 == 0
    work = torch.full((nbytes // 4 + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    src = [dev(x) for x in lams]
    outs = [_poisoned(x.size) for x in lams]
    perm = torch.full((B * F * K + PAD,), -7, dtype=torch.int32, device="cuda")
    margin = _poisoned(B * F)
    Cn, Rd, lad, Ro, lao = 0, None, None, None, None
    if Rm is not None:
        Cn = Rm[0].shape[-1]
        Rd, lad = dev(np.stack(Rm)), dev(np.stack(la))
        Ro, lao = _poisoned(B * K * F * Cn * Cn * 2), _poisoned(B * K * F)
    _lib.check(_lib.lib().pk2_perm_align(_tab(src), _lib.ptr(Rd), _lib.ptr(lad), frames, B, Cn, F, K, refine, int(noise_last),
                                         _lib.ptr(work), nbytes, _tab(outs), _lib.ptr(Ro), _lib.ptr(lao), _lib.ptr(perm),
                                         _lib.ptr(margin), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(work[nbytes // 4:].cpu().numpy()).all(), "the workspace was written beyond its size"
    p = perm.cpu().numpy()
    assert (p[B * F * K:] == -7).all() and ((p[:B * F * K] >= 0) & (p[:B * F * K] < K)).all()
    got_m = [_taken(o, x.size, "masks").reshape(x.shape) for o, x in zip(outs, lams)]
    got_R = got_la = None
    if Rm is not None:
        got_R = _taken(Ro, B * K * F * Cn * Cn * 2, "R").view(np.complex64).reshape(B, K, F, Cn, Cn)
        got_la = _taken(lao, B * K * F, "log_alpha").reshape(B, K, F)
    return got_m, got_R, got_la, p[:B * F * K].reshape(B, F, K), _taken(margin, B * F, "margin").reshape(B, F)


def _decided(lam, want):
    """the bins the comparison holds on: the restatement's margin leaves no doubt, or the bin's features are all zero, where
    every score is an exact 0 on both sides and the first candidate wins"""
    return (want["margin"] >= 1e-6) | (R.features(lam) == 0).all(axis=(1, 2))


@pytest.mark.parametrize("N", R.GPU_NS)
@pytest.mark.parametrize("F", R.GPU_FS)
@pytest.mark.parametrize("K", R.GPU_KS)
def test_aligner_against_the_restatement(K, F, N):
    lam, Rm, la, _ = R.gpu_case(K, N, F)
    want = R.align(lam, Rm)
    ok = _decided(lam, want)
    assert ok.mean() >= 0.9                       # a condition on the inputs, not a measurement
    masks, gR, gla, perm, margin = _raw_align([lam], [Rm], [la])
    assert (np.sort(perm[0], axis=1) == np.arange(K)).all()
    assert np.array_equal(perm[0][ok], want["perm"][ok])
    err = np.abs(margin[0] - want["margin"])[ok].max()
    print("K %d F %d N %d: margin error %.2e on %d of %d bins" % (K, F, N, err, ok.sum(), F))
    assert err <= MARGIN_TOL
    # everything that leaves is a gather of the input, bit for bit: by the restatement's order on the decided bins, by the
    # order the call reports on every bin
    wR, wla = R.gather_state(Rm, la, want["perm"])
    assert np.array_equal(masks[0].view(np.uint32)[:, :, ok], want["masks"].view(np.uint32)[:, :, ok])
    assert np.array_equal(gR[0][:, ok].view(np.uint32), wR[:, ok].view(np.uint32))
    assert np.array_equal(gla[0][:, ok].view(np.uint32), wla[:, ok].view(np.uint32))
    assert np.array_equal(masks[0].view(np.uint32), R.gather(lam, perm[0]).view(np.uint32))
    oR, ola = R.gather_state(Rm, la, perm[0])
    assert np.array_equal(gR[0].view(np.uint32), oR.view(np.uint32)) and np.array_equal(gla[0].view(np.uint32), ola.view(np.uint32))


@pytest.mark.parametrize("K,F,N,refine,noise_last", [(3, 33, 65, 1, True), (4, 17, 64, 8, True), (3, 33, 200, 3, False)])
def test_aligner_options(K, F, N, refine, noise_last):
    lam, Rm, la, _ = R.gpu_case(K, N, F)
    want = R.align(lam, Rm, refine=refine, noise_last=noise_last)
    ok = _decided(lam, want)
    assert ok.mean() >= 0.9
    perm, margin = _raw_align([lam], [Rm], [la], refine, noise_last)[3:]
    assert np.array_equal(perm[0][ok], want["perm"][ok]) and np.abs(margin[0] - want["margin"])[ok].max() <= MARGIN_TOL
    # without the covariances: the masks alone, in the order before the noise moves
    plain = R.align(lam, refine=refine)
    masks, gR, gla, perm, _ = _raw_align([lam], refine=refine)
    assert gR is None and np.array_equal(perm[0][ok], plain["perm"][ok])
    assert np.array_equal(masks[0].view(np.uint32), R.gather(lam, perm[0]).view(np.uint32))


def test_a_ragged_batch_equals_its_single_calls_bit_for_bit():
    K, F, frames = 3, 33, [33, 40, 98, 32]
    cases = [R.gpu_case(K, n, F) for n in frames]
    lams, Rs, las = [dev(c[0]) for c in cases], [dev(c[1]) for c in cases], [dev(c[2]) for c in cases]
    m, Ro, lao = separate.align_permutations(lams, Rs, las)
    perm, margin = separate.last_perm, separate.last_margin
    assert tuple(perm.shape) == (4, F, K) and perm.dtype == torch.int32 and tuple(margin.shape) == (4, F) and perm.is_cuda
    for i in range(4):
        mi, Ri, lai = separate.align_permutations(lams[i], Rs[i], las[i])
        assert _same(mi, m[i]) and _same(Ri, Ro[i]) and _same(lai, lao[i])
        assert torch.equal(separate.last_perm, perm[i]) and _same(separate.last_margin, margin[i])
        assert tuple(separate.last_perm.shape) == (F, K)
        want = R.align(cases[i][0], cases[i][1])
        ok = _decided(cases[i][0], want)
        assert ok.mean() >= 0.9 and np.array_equal(perm[i].cpu().numpy()[ok], want["perm"][ok])
    m2, Ro2, lao2 = separate.align_permutations(lams, Rs, las)                     # run to run
    assert all(_same(a, b) for a, b in zip(m + Ro + lao, m2 + Ro2 + lao2)) and torch.equal(separate.last_perm, perm)
    # 35 utterances: two launches per stage; every utterance as in the batch of four, wherever it stands
    idx = [(3 * i + 1) % 4 for i in range(35)]
    m35, R35, la35 = separate.align_permutations([lams[i] for i in idx], [Rs[i] for i in idx], [las[i] for i in idx])
    assert tuple(separate.last_perm.shape) == (35, F, K)
    for j, i in enumerate(idx):
        assert _same(m35[j], m[i]) and _same(R35[j], Ro[i]) and _same(la35[j], lao[i])
        assert torch.equal(separate.last_perm[j], perm[i]) and _same(separate.last_margin[j], margin[i])
    only = separate.align_permutations(lams)                                      # without the state: a list of masks
    assert isinstance(only, list) and len(only) == 4 and tuple(only[2].shape) == (K, 98, F)


_CHAIN = {}


def _chain(case):
    """the device's blind chain on a scene, once per process: (masks, perm, margin, aligned cov, separator)"""
    if case not in _CHAIN:
        from pykaldi2_amd import simulation
        b = R.blind(case)
        sep = separate.CgmmSeparator(simulation.SpectrumAnalyzer(do_dither=False), case[3], R.BLIND_ITERS)
        m = sep.masks(dev(b["Y"]))
        _CHAIN[case] = (m, sep.last_perm.cpu().numpy(), sep.last_margin.cpu().numpy(), sep.last_cov, sep)
    return _CHAIN[case]


@pytest.mark.parametrize("case", R.BLIND)
def test_the_blind_chain_against_the_restatement(case):
    Cn, N, F, S, _ = case
    b = R.blind(case)
    want = b["al"]
    ok = want["margin"] >= 0.02
    assert ok.mean() >= 0.9                       # a condition on the scenes
    m, perm, margin, cov, sep = _chain(case)
    assert tuple(m.shape) == (S + 1, N, F) and m.dtype == torch.float32 and tuple(cov.shape) == (S + 1, F, Cn, Cn)
    assert sep.last_nonfinite.tolist() == [0] and tuple(sep.last_ll.shape) == (R.BLIND_ITERS,)
    assert np.array_equal(perm[ok], want["perm"][ok])
    assert np.array_equal(perm[ok][:, S], want["perm"][ok][:, S])          # the same stream is the noise
    err = np.abs(m.cpu().numpy() - want["masks"])[:, :, ok].max()
    print(case, "aligned masks: error %.2e on %d of %d bins, smallest margin %.3f (the restatement's %.3f)"
          % (err, ok.sum(), F, margin[ok].min(), want["margin"][ok].min()))
    assert err <= BLIND_MASK_TOL
    # the same call through the functions, and the start it came from
    Y = dev(b["Y"])
    other = cgmm.cgmm_masks(Y, S + 1, R.BLIND_ITERS, init="random", seed=1)
    again = cgmm.cgmm_masks(Y, S + 1, R.BLIND_ITERS, init=dev(R.random_init(S + 1, N, F, 0)))
    blind = cgmm.cgmm_masks(Y, S + 1, R.BLIND_ITERS, init="random", seed=0)
    assert _same(blind, again) and not _same(blind, other)
    raw_cov, raw_la = cgmm.last_cov, cgmm.last_log_alpha
    am, acov, ala = separate.align_permutations(blind, raw_cov, raw_la)
    assert _same(am, m) and _same(acov, cov) and np.array_equal(separate.last_perm.cpu().numpy(), perm)
    wR, wla = R.gather_state(raw_cov.cpu().numpy(), raw_la.cpu().numpy(), perm)
    assert np.array_equal(acov.cpu().numpy().view(np.uint32), wR.view(np.uint32))
    assert np.array_equal(ala.cpu().numpy().view(np.uint32), wla.view(np.uint32))
    two = cgmm.cgmm_masks([Y, Y], S + 1, 2, init="random", seed=0)
    assert _same(two[0], cgmm.cgmm_masks(Y, S + 1, 2, init="random", seed=0))
    assert _same(two[1], cgmm.cgmm_masks(Y, S + 1, 2, init=dev(R.random_init(S + 1, N, F, 0, 1))))


@pytest.mark.parametrize("case", R.BLIND)
def test_separate_gives_every_speaker_its_stream(case):
    Cn, N, F, S, _ = case
    b = R.blind(case)
    ref_gain, assign = R.stream_gains(b["Y"], b["img"], R.separate(b["Y"], b["al"]["masks"], S))
    m = _chain(case)[0]
    Y = dev(b["Y"])
    streams = separate.separate(Y, m)
    assert len(streams) == S and all(tuple(x.shape) == (N, F) and x.dtype == torch.complex64 for x in streams)
    own = [R.si_sdr(b["Y"][0], b["img"][s, 0]) for s in range(S)]
    gain = [R.si_sdr(streams[assign[s]].cpu().numpy(), b["img"][s, 0]) - own[s] for s in range(S)]
    print(case, "SI-SDR gain per speaker over channel 0: %s dB (the restatement's %s dB)"
          % (np.round(gain, 2), np.round(ref_gain, 2)))
    assert all(g >= r - 0.5 for g, r in zip(gain, ref_gain)) and min(ref_gain) >= 3.0
    both = separate.separate([Y, Y], [m, m])
    assert len(both) == 2 and all(_same(both[i][s], streams[s]) for i in range(2) for s in range(S))


def test_dump_loglikes_writes_one_matrix_per_stream(tmp_path):
    from pykaldi2_amd import data, fbank, kaldi_io
    import yaml
    cfg = dict(data_config=dict(simulation_prob=0),
               model_config=dict(feat_dim=80, hidden_size=64, dropout=0.1, num_layers=2, label_size=120))
    cfg_path, ark = str(tmp_path / "cfg.yaml"), str(tmp_path / "out.ark")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "dump_loglikes.py"), "-config", cfg_path, "-synthetic", "2",
                          "-array_frontend", "wpe_sep_mvdr", "-num_speakers", "2", "-out_file", ark],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    source = data.SyntheticSource(120, seed=11)
    utts = [source.draw() for _ in range(2)]
    got = dict(kaldi_io.read_matrix_ark(ark))
    assert sorted(got) == sorted("%s_s%d" % (u[3], s) for u in utts for s in range(2))
    for u in utts:
        a, b = got[u[3] + "_s0"], got[u[3] + "_s1"]
        assert a.shape == b.shape == (fbank.num_frames(u[0].shape[0]), 120) and np.isfinite(a).all() and np.isfinite(b).all()
        assert not np.array_equal(a, b)


_EXISTING_KINDS = """
import sys
import numpy as np, torch
from pykaldi2_amd import cgmm
assert 'pykaldi2_amd.separate' not in sys.modules
r = np.random.RandomState(5)
wavs = [torch.from_numpy(r.standard_normal((4, n)).astype(np.float32)).cuda() for n in (6000, 4100)]
before = [x.cpu().numpy() for x in cgmm.ArrayFrontEnd('mvdr')(wavs)]
assert 'pykaldi2_amd.separate' not in sys.modules
from pykaldi2_amd import separate
streams = cgmm.ArrayFrontEnd('sep_mvdr', iterations=3)(wavs)
assert len(streams) == 2 and all(len(s) == 2 for s in streams)
assert all(tuple(y.shape) == (x.shape[1],) and bool(torch.isfinite(y).all()) for s, x in zip(streams, wavs) for y in s)
one = cgmm.ArrayFrontEnd('sep_mvdr')([wavs[0][:1]])
assert len(one) == 1 and len(one[0]) == 1 and torch.equal(one[0][0], wavs[0][0])
after = [x.cpu().numpy() for x in cgmm.ArrayFrontEnd('mvdr')(wavs)]
assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))
fe = cgmm.ArrayFrontEnd('mvdr')
assert fe.estimator.iterations == 10 and not fe.separates and fe.dereverb is None
print('UNCHANGED')
"""


def test_the_existing_kinds_are_left_as_they_were():
    out = subprocess.run([sys.executable, "-c", _EXISTING_KINDS], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "UNCHANGED" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_argument_errors():
    m = torch.full((3, 5, 17), 1 / 3, device="cuda")
    Rm = torch.zeros(3, 17, 2, 2, dtype=torch.complex64, device="cuda")
    la = torch.zeros(3, 17, device="cuda")
    Y = torch.zeros(2, 5, 17, dtype=torch.complex64, device="cuda")
    for bad, word in ((m.double(), "float32"), (m.cpu(), "CUDA"), (m[0], r"\(K, N, F\)"), (m[:1], "classes"),
                      (torch.zeros(5, 5, 17, device="cuda"), "classes"), ([m, m[:, :, :9]], "first one")):
        with pytest.raises(ValueError, match=word):
            separate.align_permutations(bad)
    for kw, word in ((dict(refine=0), "refine"), (dict(refine=9), "refine"), (dict(refine=True), "refine"),
                     (dict(noise_last=1), "noise_last"), (dict(cov=Rm), "together"), (dict(log_alpha=la), "together"),
                     (dict(cov=Rm[:2], log_alpha=la[:2]), "covariances"), (dict(cov=[Rm], log_alpha=[la]), "all lists"),
                     (dict(cov=Rm, log_alpha=la[:, :9]), "log_alpha")):
        with pytest.raises(ValueError, match=word):
            separate.align_permutations(m, **kw)
    with pytest.raises(ValueError, match="frames"):
        separate.separate(Y, m[:, :4])
    with pytest.raises(ValueError, match="both"):
        separate.separate([Y], m)
    with pytest.raises(ValueError, match="ref"):
        separate.separate(Y, m, ref=2)
    with pytest.raises(ValueError, match="'random'"):
        cgmm.cgmm_masks(Y, 3, init="uniform")
    with pytest.raises(ValueError, match="seed"):
        cgmm.cgmm_masks(Y, 3, init="random", seed=-1)
    with pytest.raises(ValueError, match="need init"):
        cgmm.cgmm_masks(Y, 3)
