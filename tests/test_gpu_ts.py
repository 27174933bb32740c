"""Lattice rescoring, plain lattice posteriors and the teacher-student criterion on the device (lattice_rescore.hip, MODE 2 of
lat_fb_posteriors) against the float64 restatement of tests/ts_ref.py on the device's own exported lattices: the decodes of
tests/test_gpu_lattice.py::CASES[:3] (T = 8 / 40 / 60, P = 12 / 60 / 150), with the forward-backward's frame values in LDS,
mixed and in global memory.  The student's log-likelihoods are 2 * default_rng(100 + seed).standard_normal((T, P))."""
import numpy as np
import pytest
import torch

import mwe_ref
import ts_ref
from oracle import lattice_ref as lr
from pykaldi2_amd import lattice, ops, synth
from test_gpu_mwe import _same

pytestmark = pytest.mark.gpu

FRAME_VALUES = ["lds", "mixed", "global_memory"]
OTHER = ("tok_frame", "tok_state", "tok_cost", "tok_final", "link_src", "link_dst", "link_tid", "link_graph")


def _cap(frame_values, monkeypatch):
    if frame_values != "lds":      # frames with more tokens than the LDS array holds are accumulated in global memory
        monkeypatch.setenv("PK2_LAT_FIN_CAP", "0" if frame_values == "global_memory" else "60")


def _recognizer(case, g, tm):
    nw, P, T, seed, beam, lb, ac, maxa, mina = case
    o = lattice.LatticeFasterDecoderOptions(beam=beam, lattice_beam=lb, max_active=maxa, min_active=mina)
    return lattice.MappedLatticeFasterRecognizer(lattice.TransitionModel.from_arrays(tm), g, ac, o)


def _decoded(case):
    g, tm, ll_T, ll_S = ts_ref.setup(case)
    rec = _recognizer(case, g, tm)
    lat = rec.decode(torch.from_numpy(ll_T).cuda())
    assert lat.status[0] == 0
    return g, tm, rec, lat, ll_T, ll_S


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _links(E):
    """The links of an export in an order that does not depend on the decode: (src, dst, tid, graph bits, acoustic bits)."""
    u32 = lambda k: np.ascontiguousarray(E[k], np.float32).view(np.uint32).tolist()
    return sorted(zip(E["link_src"].tolist(), E["link_dst"].tolist(), E["link_tid"].tolist(), u32("link_graph"), u32("link_ac")))


@pytest.mark.parametrize("frame_values", FRAME_VALUES)
@pytest.mark.parametrize("case", ts_ref.CASES)
def test_rescore_is_exact(case, frame_values, monkeypatch):
    _cap(frame_values, monkeypatch)
    for old in (0.0, 1.0, 0.5):
        g, tm, rec, lat, ll_T, ll_S = _decoded(case)
        before = lat.export(0)
        assert not lat.rescored
        lat.rescore(torch.from_numpy(ll_S).cuda().unsqueeze(0), old)
        assert lat.rescored
        after = lat.export(0)
        want = ts_ref.rescore(before, ll_S, tm["tid2pdf"], old)
        assert (before["link_tid"] > 0).sum() >= case[2]
        assert _bits(after["link_ac"]) == _bits(want)
        for k in OTHER:
            assert _bits(after[k]) == _bits(before[k]), k
    # a time-major student tensor gives what a contiguous one gives (two utterances: the layouts differ)
    P, T, seed = case[1], case[2], case[3]
    two_T = torch.from_numpy(np.stack([ll_T, ll_T])).cuda()
    two_S = np.stack([ll_S, ts_ref.student_loglikes(T, P, seed + 1)])
    tmajor = torch.from_numpy(np.ascontiguousarray(two_S.transpose(1, 0, 2))).cuda().transpose(0, 1)
    assert tmajor.stride(0) < tmajor.stride(1)
    # (two decodes may leave the links of a segment in different orders: each export against the rule on its own export
    # before, and the two link for link in a canonical order)
    a = rec.decode_batch(two_T, [T, T])
    a0 = [a.export(n) for n in range(2)]
    a.rescore(torch.from_numpy(two_S).cuda(), 0.5)
    b = rec.decode_batch(two_T, [T, T])
    b0 = [b.export(n) for n in range(2)]
    b.rescore(tmajor, 0.5)
    for n in range(2):
        ea, eb = a.export(n), b.export(n)
        assert _bits(ea["link_ac"]) == _bits(ts_ref.rescore(a0[n], two_S[n], tm["tid2pdf"], 0.5))
        assert _bits(eb["link_ac"]) == _bits(ts_ref.rescore(b0[n], two_S[n], tm["tid2pdf"], 0.5))
        assert _links(ea) == _links(eb)


@pytest.mark.parametrize("frame_values", FRAME_VALUES)
@pytest.mark.parametrize("case", ts_ref.CASES)
def test_plain_posteriors_match_restatement(case, frame_values, monkeypatch):
    _cap(frame_values, monkeypatch)
    g, tm, rec, lat, ll_T, ll_S = _decoded(case)
    E = lat.export(0)
    P, T = case[1], case[2]
    for kappa in (1.0, 0.2):
        like, post = lat.posteriors(1.0, kappa)
        wl, wp = ts_ref.posteriors(E, tm["tid2pdf"], P, 1.0, kappa)
        got = post[0].cpu().numpy().astype(np.float64)
        print("kappa %.1f: lat_like %.12f (want %.12f), max |post - want| %.3e" % (kappa, like.item(), wl, np.abs(got - wp).max()))
        assert abs(like.item() - wl) <= 1e-9 * max(1.0, abs(wl))
        assert np.abs(got - wp).max() <= 2e-6
        assert got.shape == (T, P) and np.abs(got.sum(axis=1) - 1.0).max() <= 1e-4
    assert not lat.rescored


def _check_ts(lat, E, ll_S, tm, P, kappa, old=0.0):
    loss, grad = lat.teacher_student(torch.from_numpy(ll_S).cuda().unsqueeze(0), 1.0, kappa, old)
    w = ts_ref.teacher_student(E, ll_S, tm["tid2pdf"], P, 1.0, kappa, old)
    like_T, like_S = lat.like_T.item(), lat.like_S.item()
    G = grad[0].cpu().numpy().astype(np.float64)
    print("kappa %.1f: like_T %.10f (%.10f) like_S %.10f (%.10f) loss %.12f (%.12f) max |grad - want| %.3e" % (
        kappa, like_T, w["tot_T"], like_S, w["tot_S"], loss.item(), w["loss"], np.abs(G - w["grad"]).max()))
    assert abs(like_T - w["tot_T"]) <= 1e-9 * max(1.0, abs(w["tot_T"]))
    assert abs(like_S - w["tot_S"]) <= 1e-9 * max(1.0, abs(w["tot_S"]))
    assert abs(loss.item() - w["loss"]) <= 3e-9 * max(1.0, abs(w["tot_T"]), abs(w["tot_S"]))
    assert np.abs(G - w["grad"]).max() <= 4e-6
    assert lat.rescored and loss.dtype == torch.float64 and grad.dtype == torch.float32
    return loss.item(), G, w


@pytest.mark.parametrize("frame_values", FRAME_VALUES)
@pytest.mark.parametrize("case", ts_ref.CASES)
def test_teacher_student_matches_restatement(case, frame_values, monkeypatch):
    _cap(frame_values, monkeypatch)
    P = case[1]
    for kappa in (1.0, 0.2):
        g, tm, rec, lat, ll_T, ll_S = _decoded(case)
        E = lat.export(0)
        loss, G, w = _check_ts(lat, E, ll_S, tm, P, kappa)
        assert loss > 0.0
        # the lattice is left rescored
        assert _bits(lat.export(0)["link_ac"]) == _bits(w["link_ac"])
        # again on a freshly decoded batch
        lat2 = rec.decode(torch.from_numpy(ll_T).cuda())
        loss2, G2, _ = _check_ts(lat2, lat2.export(0), ll_S, tm, P, kappa)
        assert abs(loss2 - loss) <= 3e-9 * max(1.0, abs(w["tot_T"]), abs(w["tot_S"]))
        assert np.abs(G2 - G).max() <= 4e-6


@pytest.mark.parametrize("frame_values", FRAME_VALUES)
@pytest.mark.parametrize("case", ts_ref.CASES)
def test_identity(case, frame_values, monkeypatch):
    """The new scores added to the old ones (old_acoustic_scale = 1), and the new ones zero: nothing changes."""
    _cap(frame_values, monkeypatch)
    g, tm, rec, lat, ll_T, ll_S = _decoded(case)
    before = lat.export(0)
    for kappa in (1.0, 0.2):
        loss, grad = lat.teacher_student(torch.zeros(1, case[2], case[1], device="cuda"), 1.0, kappa, 1.0)
        tot_T = lat.like_T.item()
        print("kappa %.1f: loss %.3e, max |grad| %.3e, tot_T %.6f" % (kappa, loss.item(), grad.abs().max().item(), tot_T))
        assert abs(loss.item()) <= 3e-9 * max(1.0, abs(tot_T))
        assert grad.abs().max().item() <= 4e-6
        assert _bits(lat.export(0)["link_ac"]) == _bits(before["link_ac"])


@pytest.mark.parametrize("kappa", [1.0, 0.2])
def test_gradient_descends(kappa):
    """The sign test.  The loss is convex in the student's scores with Hessian kappa^2 Cov_S(n), |n|^2 = T: a step of
    1 / (kappa T) along the returned gradient (= the loss's divided by kappa) is a 1 / L step, which lowers the loss every
    time (the float64 restatement: by at least 0.035 per step here; float32 noise is five orders below)."""
    case = ts_ref.CASES[1]
    g, tm, ll_T, ll_S = ts_ref.setup(case)
    rec = _recognizer(case, g, tm)
    T = case[2]
    teacher = torch.from_numpy(ll_T).cuda().unsqueeze(0)
    ll = torch.from_numpy(ll_S).cuda().unsqueeze(0).requires_grad_(True)
    losses = []
    for _ in range(6):
        loss = ops.TeacherStudentBatch.apply(teacher, ll, [T], rec, 1.0, kappa, 0.0)
        losses.append(loss.grad_fn.per_sequence[0].item())
        ll.grad = None
        loss.backward()
        with torch.no_grad():
            ll -= ll.grad / (kappa * T)
    print("kappa %.1f: losses %s" % (kappa, ["%.6f" % v for v in losses]))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] > 0.0


def test_ragged_batch_and_ops():
    case = ts_ref.CASES[1]
    g, tm, _, _ = ts_ref.setup(case)
    rec = _recognizer(case, g, tm)
    P, lens = case[1], [40, 17, 29]
    rng = np.random.default_rng(11)
    lls_T = [(2.0 * rng.standard_normal((T, P))).astype(np.float32) for T in lens]
    lls_S = [(2.0 * rng.standard_normal((T, P))).astype(np.float32) for T in lens]
    xT = torch.zeros(3, max(lens), P)
    xS = torch.zeros(max(lens), 3, P)                  # the student time-major, as the BLSTM produces it
    for n in range(3):
        xT[n, :lens[n]] = torch.from_numpy(lls_T[n])
        xS[:lens[n], n] = torch.from_numpy(lls_S[n])
    pred_T = xT.cuda().requires_grad_(True)
    pred_S = xS.cuda().transpose(0, 1).requires_grad_(True)
    with pytest.raises(ValueError):
        ops.TeacherStudentBatch.apply(pred_T[:, :-1], pred_S, lens, rec)
    total = ops.TeacherStudentBatch.apply(pred_T, pred_S, lens, rec)
    per_seq = total.grad_fn.per_sequence.cpu().numpy()
    assert total.dtype == torch.float32 and total.dim() == 0 and total.grad_fn.lattice.rescored
    total.backward()
    gb = pred_S.grad.clone()
    assert pred_T.grad is None
    _, raw = rec.decode_batch(pred_T.detach(), lens).teacher_student(pred_S.detach())
    assert raw.stride() == pred_S.stride()             # laid out like the student's log-likelihoods
    singles, singles64 = 0.0, 0.0
    for n in range(3):
        t = torch.from_numpy(lls_T[n]).cuda().requires_grad_(True)
        s = torch.from_numpy(lls_S[n]).cuda().requires_grad_(True)
        loss = ops.TeacherStudentMMI.apply(t, s, rec)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        assert t.grad is None
        assert (gb[n, :lens[n]] - s.grad).abs().max().item() <= 4e-6
        assert gb[n, lens[n]:].abs().sum().item() == 0.0          # padding rows
        singles += loss.item()
        # the same utterance in float64 (the operator returns float32)
        one, _ = rec.decode(torch.from_numpy(lls_T[n]).cuda()).teacher_student(torch.from_numpy(lls_S[n]).cuda().unsqueeze(0))
        assert abs(per_seq[n] - one.item()) <= 3e-9 * max(1.0, abs(one.item()))
        assert abs(loss.item() - one.item()) <= 2.0 ** -23 * abs(one.item())
        singles64 += one.item()
    print("batch %.9f per-sequence sum %.12f singles %.12f" % (total.item(), per_seq.sum(), singles64))
    assert abs(per_seq.sum() - singles64) <= 3e-9 * abs(singles64)
    # (the operators return float32: the sums agree to the rounding of their terms on top)
    assert abs(total.item() - singles) <= (3e-9 + 4 * 2.0 ** -23) * abs(singles)
    # backward returns the saved gradient whatever grad_out is
    pred_S2 = xS.cuda().transpose(0, 1).requires_grad_(True)
    (7.0 * ops.TeacherStudentBatch.apply(pred_T, pred_S2, lens, rec)).backward()
    assert (pred_S2.grad - gb).abs().max().item() <= 4e-6
    assert pred_T.grad is None


def _ali_near_lattice(rng, E, T, P):
    ali = synth.tid_alignment(rng, T, P)
    for l in range(E["link_src"].shape[0]):
        if E["link_tid"][l] != 0 and rng.random() < 0.05:
            ali[E["tok_frame"][E["link_src"][l]]] = E["link_tid"][l]
    return ali


@pytest.mark.parametrize("frame_values", FRAME_VALUES)
@pytest.mark.parametrize("case", ts_ref.CASES)
def test_other_criteria_see_the_rescored_lattice(case, frame_values, monkeypatch):
    _cap(frame_values, monkeypatch)
    g, tm, rec, lat, ll_T, ll_S = _decoded(case)
    P, T = case[1], case[2]
    lat.rescore(torch.from_numpy(ll_S).cuda().unsqueeze(0))
    E = lat.export(0)
    ref = ts_ref.ArrayLattice(E)
    ali = _ali_near_lattice(np.random.default_rng(case[3]), E, T, P)
    for drop in (True, False):
        like, post = lat.mmi([ali], 1.0, 0.2, drop)
        wl, wp = lr.lattice_mmi(ref, ali, tm["tid2pdf"], P, 1.0, 0.2, drop)
        assert abs(like.item() - wl) < 1e-9 * max(1.0, abs(wl))
        assert np.abs(post[0].cpu().numpy() - wp).max() < 2e-6
    E["start_tok"] = ref.start_tok
    words = mwe_ref.link_words(g, E)
    for distinct in (False, True):
        got = lat.nbest(16, 1.0, case[6], "words", distinct)[0]
        assert got
        _same(got, mwe_ref.kbest(E, words, 16, 1.0, case[6], distinct))


def test_failed_utterance_gives_nan_and_zero_gradient():
    """A student that gives one frame of utterance 1 no score at all leaves its rescored lattice without a path of non-zero
    weight: loss NaN and an all-zero gradient block for it, the other utterance as if it were alone."""
    case = ts_ref.CASES[1]
    g, tm, ll_T, ll_S = ts_ref.setup(case)
    rec = _recognizer(case, g, tm)
    P, T = case[1], case[2]
    two_T = torch.from_numpy(np.stack([ll_T, ll_T])).cuda()
    dead = ll_S.copy()
    dead[T // 2] = -np.inf
    lat = rec.decode_batch(two_T, [T, T])
    loss, grad = lat.teacher_student(torch.from_numpy(np.stack([ll_S, dead])).cuda(), 1.0, 0.2)
    alone = rec.decode(torch.from_numpy(ll_T).cuda())
    want, wgrad = alone.teacher_student(torch.from_numpy(ll_S).cuda().unsqueeze(0), 1.0, 0.2)
    assert torch.isnan(loss[1]).item() and grad[1].abs().sum().item() == 0.0
    assert not np.isfinite(lat.like_S[1].item()) and abs(lat.like_T[1].item() - alone.like_T.item()) <= 1e-9 * abs(alone.like_T.item())
    assert abs(loss[0].item() - want.item()) <= 3e-9 * max(1.0, abs(alone.like_T.item()), abs(alone.like_S.item()))
    assert (grad[0] - wgrad[0]).abs().max().item() <= 4e-6 and wgrad.abs().max().item() > 0.01
