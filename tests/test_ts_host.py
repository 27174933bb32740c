"""Lattice teacher-student training (ops.TeacherStudentMMI) without a GPU: the float64 restatement of tests/ts_ref.py on
oracle.lattice_ref.decode lattices -- the link formula of the loss against the Kullback-Leibler divergence of the path
distributions, its gradient against central differences, the identity case -- and the public signatures."""
import functools
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import ts_ref
from pykaldi2_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [(1.0, 1.0), (1.0, 0.2)]


@functools.lru_cache(maxsize=None)
def _case(i):
    case = ts_ref.CASES[i]
    _, tm, _, ll_S = ts_ref.setup(case)
    return case, ts_ref.decode_ref(case), tm["tid2pdf"], ll_S


@functools.lru_cache(maxsize=None)
def _result(i, lm, kappa):
    case, A, t2p, ll_S = _case(i)
    return ts_ref.teacher_student(A, ll_S, t2p, case[1], lm, kappa, 0.0)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("i", range(3))
def test_loss_is_a_divergence_and_rows_are_distributions(i, scales):
    case = ts_ref.CASES[i]
    r = _result(i, *scales)
    assert np.isfinite(r["loss"]) and r["loss"] >= 0.0
    assert r["loss"] > 1e-3          # (the student's scores are unrelated to the teacher's)
    for post in (r["post_T"], r["post_S"]):
        assert post.shape == (case[2], case[1])
        assert np.abs(post.sum(axis=1) - 1.0).max() < 1e-12
        assert post.min() >= 0.0
    assert np.abs(r["grad"].sum(axis=1)).max() < 2e-12


@pytest.mark.parametrize("old", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("scales", SCALES)
def test_link_formula_equals_path_divergence(scales, old):
    case, A, t2p, ll_S = _case(0)
    kl, npaths = ts_ref.path_kl(A, ll_S, t2p, scales[0], scales[1], old)
    assert npaths > 1
    r = ts_ref.teacher_student(A, ll_S, t2p, case[1], scales[0], scales[1], old)
    assert abs(r["loss"] - kl) < 1e-10, (r["loss"], kl)


@pytest.mark.parametrize("i", range(3))
def test_gradient_against_central_differences(i):
    """grad = d loss / d loglike_S divided by the acoustic scale: central differences of the float64 loss at h = 0.25 on the
    five entries of largest |grad| agree with kappa * grad to 1e-3 relative.
    Taken at MMI's acoustic scale, 0.2: along one entry the loss is linear plus log Z_S, whose k-th derivative is kappa^k
    times the k-th cumulant of the indicator "the path takes this pdf at this frame"; the third cumulant p (1 - p) (1 - 2 p)
    is at most 0.0963, so the scheme's own error h^2 f''' / 6 is at most 0.016 h^2 kappa^3 = 8e-6, below 1e-3 kappa |grad|
    wherever |grad| >= 0.04 (asserted).  At kappa = 1 the same term is 1e-3 absolute: the scheme, not the formula, would
    miss the bound (measured there: agreement to 3 digits)."""
    case, A, t2p, ll_S = _case(i)
    lm, kappa = 1.0, 0.2
    g = _result(i, lm, kappa)["grad"]
    h = 0.25
    for flat in np.argsort(-np.abs(g), axis=None)[:5]:
        t, pdf = np.unravel_index(flat, g.shape)
        assert abs(g[t, pdf]) >= 0.04
        hi, lo = ll_S.copy(), ll_S.copy()
        hi[t, pdf] = np.float32(ll_S[t, pdf] + np.float32(h))
        lo[t, pdf] = np.float32(ll_S[t, pdf] - np.float32(h))
        step = float(hi[t, pdf]) - float(lo[t, pdf])
        d = (ts_ref.teacher_student(A, hi, t2p, case[1], lm, kappa)["loss"] -
             ts_ref.teacher_student(A, lo, t2p, case[1], lm, kappa)["loss"]) / step
        print("case %d kappa %.1f (%d, %d): central difference %.8f, kappa * grad %.8f" % (i, kappa, t, pdf, d, kappa * g[t, pdf]))
        assert abs(d - kappa * g[t, pdf]) <= 1e-3 * abs(kappa * g[t, pdf])


@pytest.mark.parametrize("i", range(3))
def test_rescoring_with_zeros_on_top_of_the_old_scores_changes_nothing(i):
    case, A, t2p, ll_S = _case(i)
    zeros = np.zeros_like(ll_S)
    ac = ts_ref.rescore(A, zeros, t2p, 1.0)
    assert ac.dtype == np.float32 and ac.tobytes() == np.asarray(A["link_ac"], np.float32).tobytes()
    for lm, kappa in SCALES:
        r = ts_ref.teacher_student(A, zeros, t2p, case[1], lm, kappa, 1.0)
        assert r["loss"] == 0.0 and r["tot_T"] == r["tot_S"]
        assert not r["grad"].any()


def test_rescoring_rule_is_float32_and_leaves_epsilon_links_alone():
    case, A, t2p, ll_S = _case(1)
    eps = A["link_tid"] == 0
    fr = A["tok_frame"][A["link_src"]]
    for old in (0.0, 1.0, 0.5):
        ac = ts_ref.rescore(A, ll_S, t2p, old)
        assert np.array_equal(ac[eps], A["link_ac"][eps]) and not ac[eps].any()
        for l in np.flatnonzero(~eps)[::7]:
            x = ll_S[fr[l], t2p[A["link_tid"][l]]]
            want = -x if old == 0.0 else np.float32(np.float32(np.float32(old) * A["link_ac"][l]) - x)
            assert ac[l] == want


def test_operators_have_the_documented_signatures():
    assert list(inspect.signature(ops.TeacherStudentMMI.forward).parameters) == ["ctx", "loglikes_T", "loglikes_S", "asr_decoder"]
    sig = inspect.signature(ops.TeacherStudentBatch.forward)
    assert list(sig.parameters) == ["ctx", "prediction_T", "prediction_S", "lengths", "asr_decoder", "lm_scale", "acoustic_scale",
                                    "old_acoustic_scale"]
    assert [sig.parameters[k].default for k in ("lm_scale", "acoustic_scale", "old_acoustic_scale")] == [1.0, 1.0, 0.0]
    from pykaldi2_amd import lattice, se
    sig = inspect.signature(lattice.LatticeBatch.teacher_student)
    assert list(sig.parameters) == ["self", "loglikes_S", "lm_scale", "acoustic_scale", "old_acoustic_scale"]
    assert list(inspect.signature(lattice.LatticeBatch.rescore).parameters) == ["self", "loglikes", "old_acoustic_scale"]
    assert list(inspect.signature(lattice.LatticeBatch.posteriors).parameters) == ["self", "lm_scale", "acoustic_scale"]
    assert callable(se.sequence_loss_ts)


def test_ts_settings_defaults_and_unknown_keys():
    from pykaldi2_amd import se
    assert se.ts_settings({}, 0.3) == dict(lm_weight=1.0, am_weight=0.3, old_acoustic_scale=0.0)
    assert se.ts_settings({"ts_config": {"am_weight": 1.0, "old_acoustic_scale": 1}}, 0.3) == dict(
        lm_weight=1.0, am_weight=1.0, old_acoustic_scale=1.0)
    with pytest.raises(KeyError):
        se.ts_settings({"ts_config": {"num_paths": 4}}, 0.3)


def test_train_se2_help_lists_the_criterion_and_the_teacher():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "train_se2.py"), "-h"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "-teacher_model" in out.stdout
    choices = out.stdout[out.stdout.index("-criterion"):]
    assert "ts" in choices[choices.index("{"):choices.index("}")].split(",")
