"""The frequency permutation aligner and the blind separation front end without a GPU: properties of the float64
restatement (tests/perm_align_ref.py), the conditions the GPU tests rely on (margins, the float32 mode's error), the seeded
random start of cgmm_masks, the argument checks that run before the device is touched, and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perm_align_ref as R  # noqa: E402

from pykaldi2_amd import _lib, cgmm, separate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRAMBLED = [(K, N, F) for K in R.KS for N in R.NS for F in R.FS]


def test_constants_match_the_header():
    assert (separate.MAX_CLASSES, separate.MAX_REFINE, separate.MAX_SPEAKERS) == (4, 8, 3)
    assert "#define PK2_PERM_ALIGN_MAX_REFINE 8\n" in open(os.path.join(ROOT, "include", "pk2hip.h")).read()
    assert cgmm.FRONT_ENDS == ("none", "mvdr", "wpe_mvdr", "sep_mvdr", "wpe_sep_mvdr")


def test_best_takes_the_first_maximum_in_lexicographic_order():
    assert R.perms(3).tolist() == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]]
    p, top, second = R.best(np.zeros((3, 3)))
    assert p.tolist() == [0, 1, 2] and top == 0 and second == 0
    S = np.array([[0.0, 1.0], [1.0, 0.0]])
    p, top, second = R.best(S)
    assert p.tolist() == [1, 0] and top == 2 and second == 0
    S = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])      # (0, 1, 2) and (1, 0, 2) tie at 3
    assert R.best(S)[0].tolist() == [0, 1, 2]


@pytest.mark.parametrize("K,N,F", SCRAMBLED)
def test_scrambled_masks_come_back_in_one_order(K, N, F):
    lam, truth = R.scrambled(K, N, F, 0)
    clean = R.gather(lam, np.argsort(truth, axis=1))
    assert ((clean[:K - 1].mean(axis=2) < 0.2).mean(axis=1) >= 0.25).all()      # every speaker is silent on a quarter of the frames
    assert not (truth == truth[0]).all()
    a = R.align(lam)
    print("K %d N %d F %d: smallest margin %.3f" % (K, N, F, a["margin"].min()))
    assert (a["margin"] >= 0.05).all()          # the condition: the inputs leave no doubt, in the restatement alone
    assert R.consistent(a["perm"], truth).all()
    assert np.array_equal(a["masks"], R.gather(lam, a["perm"]))
    assert sorted(a["perm"][0].tolist()) == list(range(K)) and (np.sort(a["perm"], axis=1) == np.arange(K)).all()


@pytest.mark.parametrize("K,N,F", [(3, 33, 33), (4, 64, 65)])
def test_few_frames_and_an_odd_group_at_every_level(K, N, F):
    """fewer frames than a wave, and F = 2^k + 1; the figure without the tree stage is printed for comparison"""
    lam, truth = R.scrambled(K, max(N, 64), F, 3)
    lam = lam[:, :N]
    with_tree = R.consistent(R.align(lam)["perm"], truth).mean()
    without = R.consistent(R.align(lam, tree=False, refine=1)["perm"], truth).mean()
    print("K %d N %d F %d: consistent bins with the tree %.2f, without it after one round %.2f" % (K, N, F, with_tree, without))
    assert with_tree >= 0.9 and with_tree >= without


@pytest.mark.parametrize("K,N,F", [(2, 64, 17), (3, 98, 33), (4, 200, 257)])
def test_aligning_twice_gives_the_same_streams(K, N, F):
    lam, _ = R.scrambled(K, N, F, 1)
    first = R.align(lam)["masks"]
    again = R.gather(first, np.stack([np.random.RandomState(f).permutation(K) for f in range(F)]))
    second = R.align(again)["masks"]
    # one global relabelling: every stream of the second run is, whole, a stream of the first
    match = [[np.array_equal(second[a], first[b]) for b in range(K)] for a in range(K)]
    assert sorted(np.argmax(match, axis=1).tolist()) == list(range(K)) and np.sum(match) == K


def test_a_constant_bin_keeps_the_identity():
    """A constant mask has u = 0, so every score it enters is 0 and every choice made for it is the identity: constant
    masks throughout keep the identity in every bin, and so does a constant bin 0, which is in no right group.  A constant
    bin further up has nothing of its own to say either (margin 0, the refinement leaves it alone) and carries what the
    merges above it gave its group, as the mathematics of DESIGN.md 7.12 has it; the other bins are not disturbed."""
    flat = np.tile(np.array([0.5, 0.25, 0.25], np.float32)[:, None, None], (1, 98, 17))
    a = R.align(flat)
    assert (a["perm"] == np.arange(3)).all() and (a["margin"] == 0).all() and (R.features(flat) == 0).all()
    lam, truth = R.scrambled(3, 98, 17, 2)
    lam[:, :, 0] = np.float32(1 / 3)
    lam[:, :, 5] = np.float32(1 / 3)
    lam[:, :, 11] = np.array([0.5, 0.25, 0.25], np.float32)[:, None]
    a = R.align(lam)
    assert a["perm"][0].tolist() == [0, 1, 2]
    assert a["margin"][0] == 0 and a["margin"][5] == 0 and a["margin"][11] == 0
    assert np.array_equal(a["perm"][[5, 11]], R.align(lam, refine=1)["perm"][[5, 11]])
    rest = np.ones(17, bool)
    rest[[0, 5, 11]] = False
    assert R.consistent(a["perm"][rest], truth[rest]).all() and (a["margin"][rest] >= 0.05).all()
    assert (R.features(lam)[[0, 5, 11]] == 0).all()


@pytest.mark.parametrize("K", R.KS)
def test_one_frame_keeps_the_identity_everywhere(K):
    lam = R._small(K, 1, 33)[0]
    a = R.align(lam)
    assert (a["perm"] == np.arange(K)).all() and (a["margin"] == 0).all() and np.array_equal(a["masks"], lam)


def test_the_smallest_purity_sum_goes_last():
    for K, N, F in ((2, 64, 17), (3, 98, 33), (4, 200, 17)):
        lam, Rm, la, truth = R.gpu_case(K, N, F)
        a = R.align(lam, Rm)
        plain = R.align(lam)
        assert a["noise"] == int(np.argmin(a["q"])) and np.sort(a["q"])[1] > 1.5 * a["q"].min()
        order = [s for s in range(K) if s != a["noise"]] + [a["noise"]]
        assert np.array_equal(a["perm"], plain["perm"][:, order])
        # the flat class of every bin is the one that ends last
        assert (np.take_along_axis(truth, a["perm"], 1)[:, K - 1] == K - 1).all()
        assert R.align(lam, Rm, noise_last=False)["noise"] is None
    q_tie = R.align(lam, np.tile(np.eye(3, dtype=np.complex64), (K, F, 1, 1)))
    assert q_tie["noise"] == 0 and q_tie["perm"][0].tolist() == plain["perm"][0][[1, 2, 3, 0]].tolist()


def test_the_blind_scenes_meet_the_conditions_of_the_gpu_test():
    for case in R.BLIND:
        b = R.blind(case)
        al, S = b["al"], case[3]
        print(case, "min margin %.3f, q %s" % (al["margin"].min(), np.round(al["q"], 2)))
        assert (al["margin"] >= 0.02).mean() >= 0.9
        assert al["noise"] == int(np.argmin(al["q"])) and np.sort(al["q"])[1] > 1.5 * al["q"].min()
        gains, _ = R.stream_gains(b["Y"], b["img"], R.separate(b["Y"], al["masks"], S))
        print(case, "SI-SDR gains %s dB" % np.round(gains, 2))
        assert min(gains) >= 3.0


def test_the_float32_mode_bounds_the_margin_error():
    worst = max(R.float32_margin_error(K, N, F) for K in R.GPU_KS for F in (17, 257) for N in (65, 200))
    print("largest margin error of the float32 mode on these cases: %.2e" % worst)
    assert 0 < worst < 1e-5


def test_the_random_start_is_reproducible_from_the_seed():
    a, b = cgmm.random_init(3, 20, 17, 0), cgmm.random_init(3, 20, 17, 0)
    assert a.dtype == np.float32 and a.shape == (3, 20, 17) and np.array_equal(a, b)
    assert np.abs(a.sum(axis=0) - 1).max() < 1e-6 and a.min() >= 0.05 / 3.2
    assert not np.array_equal(a, cgmm.random_init(3, 20, 17, 1))
    assert not np.array_equal(a, cgmm.random_init(3, 20, 17, 0, index=1))
    assert np.array_equal(a, R.random_init(3, 20, 17, 0))
    x = np.random.default_rng([0, 0]).random((3, 20, 17), np.float32) + np.float32(0.05)
    assert np.array_equal(a, (x / x.sum(axis=0, keepdims=True)).astype(np.float32))


def _err():
    return _lib.lib().pk2_last_error().lower()


def test_bad_abi_arguments_fail_loudly():
    L = _lib.lib()
    one, two = (C.c_void_p * 1)(8), (C.c_void_p * 1)(16)         # never dereferenced: every call below is refused on the host
    frames = (C.c_int32 * 1)(5)
    w, v = C.c_void_p(8), C.c_void_p(16)
    big = 1 << 26

    def run(masks=one, cov=None, la=None, fr=frames, B=1, Cn=0, F=17, K=3, refine=3, noise=1, work=w, nbytes=big, out=two,
            ocov=None, ola=None, perm=w, margin=w):
        return L.pk2_perm_align(masks, cov, la, fr, B, Cn, F, K, refine, noise, work, nbytes, out, ocov, ola, perm, margin, None)
    assert run(masks=None) < 0 and b"null" in _err()
    assert run(out=None) < 0 and b"null" in _err()
    assert run(out=(C.c_void_p * 1)(None)) < 0 and b"null" in _err()
    assert run(out=one) < 0 and b"out of place" in _err()
    assert run(B=0) < 0 and b"utterances" in _err()
    assert run(F=0) < 0 and b"bins" in _err()
    assert run(F=4098) < 0 and b"bins" in _err()
    assert run(K=1) < 0 and b"classes" in _err()
    assert run(K=5) < 0 and b"classes" in _err()
    assert run(refine=0) < 0 and b"refinement" in _err()
    assert run(refine=9) < 0 and b"refinement" in _err()
    assert run(fr=None) < 0 and b"frames" in _err()
    assert run(fr=(C.c_int32 * 1)(0)) < 0 and b"frames" in _err()
    assert run(nbytes=16) < 0 and b"workspace" in _err()
    assert run(perm=None) < 0 and b"null" in _err()
    assert run(margin=None) < 0 and b"null" in _err()
    assert run(cov=w) < 0 and b"together" in _err()
    assert run(cov=w, la=w, ocov=v) < 0 and b"together" in _err()
    assert run(cov=w, la=w, ocov=v, ola=v, Cn=9) < 0 and b"channels" in _err()
    assert run(cov=w, la=w, ocov=w, ola=v, Cn=2) < 0 and b"out of place" in _err()
    with pytest.raises(_lib.Pk2Error):
        _lib.check(run(work=None))
    need = L.pk2_perm_align_workspace_bytes(frames, 1, 17, 3)
    assert need >= 5 * 3 * 17 * 4 + 2 * 5 * 3 * 9 * 4
    assert L.pk2_perm_align_workspace_bytes(None, 1, 17, 3) == 0 and L.pk2_perm_align_workspace_bytes(frames, 0, 17, 3) == 0
    assert L.pk2_perm_align_workspace_bytes(frames, 1, 0, 3) == 0 and L.pk2_perm_align_workspace_bytes(frames, 1, 17, 5) == 0
    assert L.pk2_perm_align_workspace_bytes((C.c_int32 * 1)(0), 1, 17, 2) == 0


def test_python_argument_errors_that_need_no_gpu():
    with pytest.raises(ValueError, match="CUDA float32"):
        separate.align_permutations(np.zeros((3, 5, 17), np.float32))
    with pytest.raises(ValueError, match="empty"):
        separate.align_permutations([])
    with pytest.raises(ValueError, match="complex64"):
        separate.separate(np.zeros((2, 5, 17), np.complex64), None)
    for kw, word in ((dict(num_speakers=0), "num_speakers"), (dict(num_speakers=4), "num_speakers"),
                     (dict(iterations=0), "iterations"), (dict(refine=0), "refine"), (dict(refine=9), "refine"),
                     (dict(seed=-1), "seed"), (dict(diag_load=-1), "diag_load")):
        with pytest.raises(ValueError, match=word):
            separate.CgmmSeparator(None, **kw)
    with pytest.raises(ValueError, match="num_speakers"):
        cgmm.ArrayFrontEnd("sep_mvdr", num_speakers=4)
    with pytest.raises(ValueError, match="kind"):
        cgmm.ArrayFrontEnd("sep")
    with pytest.raises(ValueError, match="complex64"):
        cgmm.cgmm_masks(np.zeros((2, 5, 17), np.complex64), 3, init="random")


def test_the_command_line_takes_the_new_choices():
    sys.path.insert(0, os.path.join(ROOT, "bin"))
    import dump_loglikes
    p = dump_loglikes.arg_parser()
    a = p.parse_args(["-config", "c.yaml", "-array_frontend", "wpe_sep_mvdr", "-num_speakers", "3"])
    assert a.array_frontend == "wpe_sep_mvdr" and a.num_speakers == 3
    a = p.parse_args(["-config", "c.yaml", "-array_frontend", "sep_mvdr"])
    assert a.array_frontend == "sep_mvdr" and a.num_speakers == 2
    assert p.parse_args(["-config", "c.yaml"]).array_frontend == "none"
    with pytest.raises(SystemExit):
        p.parse_args(["-array_frontend", "sep"])
