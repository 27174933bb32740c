"""The lattice forward-backward (pykaldi2_amd/csrc/lattice_fb.hip) against the float64 oracle on lattices that reach the paths
of its linear-domain kernel the lattices of test_gpu_lattice.py never reach (tests/lattice_cases.py: frames beyond the register
slots, both overflow loops, frames beyond the LDS half-array with no hook, a backward recursion that starts on an epsilon
overflow), every criterion on every case, and on a lattice whose scores span more than the linear form's range.

Tolerances: likelihood / score 1e-9 relative (the project's bound); a posterior matrix max(2e-6, 4 x the deviation of a float32
accumulation of the oracle's float64 per-link terms over 8 random orders) -- lattice_cases.post_bound --, sMBR / MPFE scaled
by max(1, |want|.max()).  Every comparison prints the device's error next to its bound (DESIGN.md records them).

A recursion that leaves the linear form's range is run again in the log domain, silently.  So every comparison also asserts
which kernel's values it has checked (LatticeBatch.fb_rerun): the wide cases, CASES[:3] and the lower rungs of the range
ladder must NOT have been run again -- a fault in an overflow loop or a register slot that leaves live tokens at 0 would
otherwise be repaired by the rerun and pass --, what is beyond the range must have been."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lattice_cases as lc
import ts_ref
from oracle import lattice_ref as lr
from pykaldi2_amd import _lib, lattice
from test_gpu_lattice import CASES, _canon

pytestmark = pytest.mark.gpu

HOOKS = ["lds", "mixed", "global_memory"]       # PK2_LAT_FIN_CAP unset / 60 / 0: tokens a frame may have and stay in LDS
WIDE_HOOKED = [(n, h) for n in sorted(lc.WIDE) for h in (HOOKS if n in ("WIDE_A", "WIDE_D") else HOOKS[:1])]
KAPPAS = (1.0, 0.2)
LINEAR = os.environ.get("PK2_FB_LINEAR") != "0"     # (the child process of test_log_domain_kernel: no linear kernel, no marks)
STOOD = (0, 0)                                      # fb_rerun of an utterance whose linear alpha and beta both stood


def _hook(hook, monkeypatch):
    if hook != "lds":
        monkeypatch.setenv("PK2_LAT_FIN_CAP", "0" if hook == "global_memory" else "60")


def _decode(c):
    """Device decode of a case, held to the oracle's lattice as test_decoder_matches_oracle does."""
    beam, lb, ac, maxa, mina = c.case[4:]
    o = lattice.LatticeFasterDecoderOptions(beam=beam, lattice_beam=lb, max_active=maxa, min_active=mina)
    rec = lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(c.tm), c.g, ac, o)
    lat = rec.decode(torch.from_numpy(c.ll).cuda())
    assert lat.status[0] == 0
    assert lat.best_cost[0] == np.float32(c.want.best_cost)
    got_t, got_l = _canon(lat.export(0))
    want_t, want_l = _canon(c.A)
    assert len(got_t) == len(want_t) and len(got_l) == len(want_l), (len(got_t), len(want_t), len(got_l), len(want_l))
    assert got_t == want_t and got_l == want_l       # bit-exact token costs, identical link set with bit-exact costs
    return rec, lat


# the oracle's answers and the bounds, once per process and case (the hook settings share them)
@functools.lru_cache(maxsize=None)
def _want(name, criterion, args):
    return lc.oracle(name, criterion, args)


def _check(what, lat, value, post, want, rerun=STOOD):
    wv, wp, bound = want
    got = tuple(int(v) for v in lat.fb_rerun()[0])
    assert got == (rerun if LINEAR else (-1, -1)), (what, "alpha / beta run again in the log domain:", got)
    err_v = abs(value.item() - wv) / max(1.0, abs(wv))
    err_p = np.abs(post[0].cpu().numpy().astype(np.float64) - wp).max()
    print("%s: value %.12g (oracle %.12g, relative error %.2g, bound 1e-09); posteriors: error %.3g, bound %.3g" % (
        what, value.item(), wv, err_v, err_p, bound))
    assert err_v < 1e-9, what
    assert err_p < bound, what


def _check_all(name, lat, only=None, rerun=STOOD):
    """Every setting of the case (lattice_cases.settings) whose criterion or first argument is in `only`."""
    c = lc.case(name)
    for criterion, args in lc.settings(name):
        if only is not None and criterion not in only and args[0] not in only:
            continue
        if criterion == "mmi":
            value, post = lat.mmi([c.ali], 1.0, args[0], args[1])
        elif criterion == "posteriors":
            value, post = lat.posteriors(1.0, args[0])
        else:
            value, post = lat.mpe([c.ali], args[0], c.tm["silence_phones"], args[1])
        _check("%s %s %s" % (name, criterion, args), lat, value, post, _want(name, criterion, args), rerun)


@pytest.mark.parametrize("name,hook", WIDE_HOOKED)
def test_wide_mmi_and_posteriors_match_oracle(name, hook, monkeypatch):
    _hook(hook, monkeypatch)
    rec, lat = _decode(lc.case(name))
    _check_all(name, lat, ("mmi", "posteriors"))


@pytest.mark.parametrize("criterion", ["smbr", "mpfe"])
@pytest.mark.parametrize("name,hook", WIDE_HOOKED)
def test_wide_mpe_matches_oracle(name, hook, criterion, monkeypatch):
    _hook(hook, monkeypatch)
    rec, lat = _decode(lc.case(name))
    _check_all(name, lat, (criterion,))


@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_small_cases_mpe_matches_oracle_on_mixed_frames(i, hook, monkeypatch):
    """sMBR and MPFE on test_gpu_lattice.py::CASES[:3] with every frame in LDS, mixed, and every frame in global memory:
    lat_fb_logs on a mixture of linear and log frames."""
    _hook(hook, monkeypatch)
    name = "CASES%d" % i
    rec, lat = _decode(lc.case(name))
    _check_all(name, lat)


# ----------------------------------------------------------------------------------------------------------------------
# One ragged batch: WIDE_A's graph, lengths [5, 1, 3], and an utterance whose rescored lattice has no path.
# ----------------------------------------------------------------------------------------------------------------------
def _guarded(N, Tmax, P):
    """A zeroed [N, Tmax, P] view with a frame stride of P + 8 inside a buffer of NaNs."""
    big = torch.full((N, Tmax, P + 8), float("nan"), device="cuda")
    big[:, :, :P] = 0.0
    return big, big[:, :, :P]


def _abi(lat, what, alis, tm, post):
    """mmi / smbr / posteriors through the C ABI into a caller's post buffer -> the [N] likelihoods or scores."""
    L = _lib.lib()
    N = len(lat.lengths)
    out = torch.empty(N, dtype=torch.float64, device="cuda")
    t2p, t2ph = lat.trans_model.device_tables(lat.device)
    sp = _lib.stream_ptr(lat.device)
    if what == "posteriors":
        _lib.check(L.pk2_lattice_posteriors(lat._h, _lib.ptr(lat.workspace), _lib.ptr(t2p), 1.0, 0.2, 1.0, _lib.ptr(post),
                                            post.stride(0), post.stride(1), _lib.ptr(out), sp))
        return out
    ref = lat._ref(alis)
    if what == "mmi":
        _lib.check(L.pk2_lattice_mmi(lat._h, _lib.ptr(lat.workspace), _lib.ptr(ref), ref.stride(0), _lib.ptr(t2p), 1.0, 0.2, 0,
                                     _lib.ptr(post), post.stride(0), post.stride(1), _lib.ptr(out), sp))
    else:
        sil = lat.trans_model.silence_mask(tm["silence_phones"], lat.device)
        _lib.check(L.pk2_lattice_mpe(lat._h, _lib.ptr(lat.workspace), _lib.ptr(ref), ref.stride(0), _lib.ptr(t2p), _lib.ptr(t2ph),
                                     _lib.ptr(sil), 0, 1, 1.0, 1.0, _lib.ptr(post), post.stride(0), post.stride(1),
                                     _lib.ptr(out), sp))
    torch.cuda.synchronize()
    return out


def test_ragged_batch_with_a_failed_utterance():
    c = lc.wide("WIDE_A")
    P, lens = c.P, [5, 1, 3, 5]
    rec, _ = _decode(c)
    x = np.zeros((4, 5, P), np.float32)
    for n, T in enumerate(lens):
        x[n, :T] = c.ll[:T]
    dead = x.copy()
    dead[3, 2] = -np.inf           # no score at all on one frame: utterance 3's rescored lattice has no path of non-zero weight
    alis = [c.ali[:T] for T in lens]
    lat = rec.decode_batch(torch.from_numpy(x).cuda(), lens)
    assert (lat.status == 0).all()
    lat.rescore(torch.from_numpy(dead).cuda())
    singles = []
    for n in range(3):
        one = rec.decode(torch.from_numpy(x[n, :lens[n]]).cuda())
        one.rescore(torch.from_numpy(x[n:n + 1, :lens[n]]).cuda())
        singles.append(one)
    # the bound of an utterance: the float32 model on the oracle's lattice of the same frames
    t2p = c.tm["tid2pdf"]
    bounds = []
    for T in lens[:3]:
        k = lc.wide_cut("WIDE_A", T)
        wp = lr.lattice_mpe(k.want, k.ali, t2p, k.tm["tid2phone"], k.tm["silence_phones"], P, "smbr", True)[1]
        bounds.append({"mmi": lc.post_bound(*lc.terms_mmi(k.want, k.ali, t2p, 1.0, 0.2, False), T, P),
                       "smbr": lc.post_bound(*lc.terms_mpe(k.want, k.ali, k.tm, P, "smbr", True), T, P, max(1.0, np.abs(wp).max())),
                       "posteriors": lc.post_bound(*lc.terms_posteriors(k.want, t2p, 1.0, 0.2), T, P)})
    for what in ("mmi", "smbr", "posteriors"):
        big, post = _guarded(4, 5, P)
        out = _abi(lat, what, alis, c.tm, post).cpu().numpy()
        got = post.cpu().numpy()
        assert torch.isnan(big[:, :, P:]).all()               # nothing written between the rows
        if LINEAR:      # the live utterances stayed linear; the dead one (every token behind its dead frame is 0) was run again
            assert lat.fb_rerun().tolist() == [[0, 0], [0, 0], [0, 0], [1, 1]]
        for n in range(3):
            if what == "mmi":
                v, p1 = singles[n].mmi([alis[n]], 1.0, 0.2, False)
            elif what == "smbr":
                v, p1 = singles[n].mpe([alis[n]], "smbr", c.tm["silence_phones"], True)
            else:
                v, p1 = singles[n].posteriors(1.0, 0.2)
            err = np.abs(got[n, :lens[n]] - p1[0].cpu().numpy()).max()
            print("batch %s utterance %d: value %.12g (alone %.12g), posteriors differ by %.3g, bound %.3g" % (
                what, n, out[n], v.item(), err, bounds[n][what]))
            assert abs(out[n] - v.item()) < 1e-9 * max(1.0, abs(v.item()))
            assert err < bounds[n][what] and np.abs(p1[0].cpu().numpy()).max() > 0.01
            assert not got[n, lens[n]:].any()                  # padding frames: exactly 0
        assert np.isnan(out[3]) and not got[3].any()           # the failed utterance: NaN and a zero post row


# ----------------------------------------------------------------------------------------------------------------------
# Dynamic range (lattice_cases.two_branch_graph): branch B is X h nats behind at frame h and wins by X h at the end.
# ----------------------------------------------------------------------------------------------------------------------
# Which recursions must have left the linear form (a live token below 1e-280 of the neighbouring frame's maximum, ~645 nats):
# forward, B is X h behind at frame h; backward, A is 2 X h behind there.
RANGE_RERUN = {120: (0, 0), 300: (0, 0), 600: (0, 1), 1200: (1, 1)}


@pytest.mark.parametrize("Xh", [120, 300, 600])
def test_range_ladder_matches_oracle(Xh):
    name = "RANGE_%d" % Xh
    rec, lat = _decode(lc.case(name))
    _check_all(name, lat, ("mmi", "posteriors", "smbr"), RANGE_RERUN[Xh])


def test_scores_above_the_weight_window_match_oracle():
    """Every score raised by 50: link weights of exp(50 - graph cost) > 1e15 are not taken into the linear form (a frame's
    maximum must stay small enough for value / maximum to be a normal number); both recursions are run again in logs."""
    c = lc.range_case(10.0, 50.0)
    rec, lat = _decode(c)
    t2p = c.tm["tid2pdf"]
    like, post = lat.posteriors(1.0, 1.0)
    t, pdf, g = lc.terms_posteriors(c.want, t2p, 1.0, 1.0)
    want = ts_ref.posteriors(dict(c.A, start_tok=c.want.start_tok, T=c.T), t2p, c.P, 1.0, 1.0)
    _check("scores + 50 posteriors", lat, like, post, want + (lc.post_bound(t, pdf, g, c.T, c.P),), (1, 1))
    like, post = lat.mmi([c.ali], 1.0, 1.0, False)
    want = lr.lattice_mmi(c.want, c.ali, t2p, c.P, 1.0, 1.0, False)
    _check("scores + 50 mmi", lat, like, post, want + (lc.post_bound(*lc.terms_mmi(c.want, c.ali, t2p, 1.0, 1.0, False), c.T, c.P),),
           (1, 1))


def test_beyond_the_linear_range_matches_oracle():
    """X h = 1200: B is 1200 nats behind at mid-utterance, more than a double holds in linear form (exp(-745) = 0).  The
    oracle gives B a posterior of 1 and a total of -1197.69.  Before the linear kernel noticed what leaves its range it lost
    B near frame 8 and returned A's total, with no status: MMI likelihood -2396.64016298 against the oracle's -1197.69025473,
    posteriors of +inf.  (At X h = 600 the likelihood was right and a frame whose reference is on branch A, posterior
    exp(-600), was dropped by drop_frames although Kaldi's test is "== 0": error 1.0.)  Now a recursion that leaves the
    range is run again by the log-domain kernel, and every criterion matches."""
    c = lc.case("RANGE_1200")
    rec, lat = _decode(c)
    _check_all("RANGE_1200", lat, None, RANGE_RERUN[1200])
    # teacher-student: the lattice's own scores (out of range), then a student's whose B is behind by 1080
    ll_S = lc.two_branch_loglikes(90.0, c.branch_pdfs)
    want = ts_ref.teacher_student(lat.export(0), ll_S, c.tm["tid2pdf"], c.P, 1.0, 1.0)
    loss, grad = lat.teacher_student(torch.from_numpy(ll_S).cuda().unsqueeze(0), 1.0, 1.0)
    bound = sum(lc.post_bound(*lc.terms_posteriors(ts_ref.ArrayLattice(dict(c.A, start_tok=c.want.start_tok, T=c.T), ac),
                                                    c.tm["tid2pdf"], 1.0, 1.0), c.T, c.P)
                for ac in (None, ts_ref.rescore(c.A, ll_S, c.tm["tid2pdf"])))
    err = np.abs(grad[0].cpu().numpy() - want["grad"]).max()
    if LINEAR:
        assert lat.fb_rerun().tolist() == [[1, 1]]       # (the student's pass: B 1080 behind)
    print("X h = 1200 teacher-student: like_T %.12g (oracle %.12g), like_S %.12g (oracle %.12g), loss %.6g (oracle %.6g), "
          "gradient error %.3g, bound %.3g" % (lat.like_T.item(), want["tot_T"], lat.like_S.item(), want["tot_S"], loss.item(),
                                                 want["loss"], err, bound))
    assert abs(lat.like_T.item() - want["tot_T"]) < 1e-9 * abs(want["tot_T"])
    assert abs(lat.like_S.item() - want["tot_S"]) < 1e-9 * abs(want["tot_S"])
    assert abs(loss.item() - want["loss"]) < 3e-9 * max(1.0, abs(want["tot_T"]), abs(want["tot_S"]))
    assert err < bound


def test_log_domain_kernel():
    """PK2_FB_LINEAR=0 (read once per process, hence the child): the log-domain kernel, the documented fallback, passes the
    oracle comparisons of this file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_lattice_fb.py"), "-q", "-m", "gpu",
                          "-k", "oracle"], env=dict(os.environ, PK2_FB_LINEAR="0"), capture_output=True, text=True,
                         timeout=900, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
