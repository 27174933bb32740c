"""Every LSTM recurrence path straight through the C ABI (pk2_lstm_layer_fwd / _bwd / _bwd_bias) against the float64 layer
oracle of oracle/lstm_ref.py, one case at a time: which kernels ran (pk2_lstm_last_path), every output element written
and finite, nothing written outside the tensors, the documented += of the bias gradients, bit-reproducibility, and

    max |X_device - X_float64|  <=  4 * max(e32(X), 2^-23 max |X_float64|)     for X in y, gates, cells, dgx, dbias

with e32(X) the error of the float32 oracle on the same data (tests/lstm_check.py; the bound is never taken from the
kernels).  Paths (include/pk2hip.h, PK2_LSTM_PATH_*): SEQ lstm_fwd_seq2 / lstm_bwd_seq2, BIG lstm_fwd_big_persist /
lstm_bwd_big_persist2, BIG_AG lstm_bwd_big_persist, STEP_SMALL lstm_fwd_step / lstm_bwd_step_x4, STEP_BIG
lstm_fwd_step_big / lstm_bwd_dh_big + lstm_bwd_pointwise_big.  Two data regimes per case (lstm_check.make_case): linear,
and saturated (gates at exactly 0 and 1, |c| up to 7, exp2 overflowing inside both nonlinearities).

Measured on the MI355X ("Layer-level pins": largest device error / max(e32, floor) per path, tensor and
regime) the worst line is STEP_BIG forward, gates: 2.90 linear / 2.57 saturated (B = 32, T = 2, H = 1024, D = 2); no path
needs more than the common factor 4.

Which repeated backward calls must be bit-identical is decided from the code, not by trying: d gx is summed in an order
fixed by construction on every path (MFMA accumulators, DPP row sums and mailbox slots read in rank order, split-K
partials added s = 0..3); the ONLY float atomics of the recurrences are the bias gradients of lstm_bwd_seq2 (one
atomicAdd per gate row and (sequence, direction) pair, csrc/lstm_persist_seq.hip), so dbias_ih / dbias_hh of SEQ with
more than one sequence are exempt from bit-identity (they are still held to the bound); everything else is not.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_check
from pykaldi2_amd import _lib

pytestmark = pytest.mark.gpu

NONE, SEQ, BIG, BIG_AG, STEP_SMALL, STEP_BIG = range(6)       # PK2_LSTM_PATH_* of include/pk2hip.h
PATH_NAME = ["NONE", "SEQ", "BIG", "BIG_AG", "STEP_SMALL", "STEP_BIG"]
# (path, tensor) -> factor, for a path that needs more than lstm_check.FACTOR on a tensor: only with the arithmetic step
# that costs it named here, and never past 16.
FACTORS = {}

BAND, CANARY = 64, 1234.5


class Guarded:
    """A device tensor of n floats inside a larger allocation, a band of 64 floats of a fixed finite value in front of it
    and behind it.  misalign = 1: the tensor starts one float further on (4-byte aligned, not 16)."""

    def __init__(self, data=None, n=None, fill=float("nan"), misalign=0):
        self.host = None if data is None else np.ascontiguousarray(data, np.float32)
        self.n = int(n if data is None else self.host.size)
        self.front = BAND + misalign
        self.buf = torch.full((self.front + self.n + BAND,), CANARY, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.front:self.front + self.n]
        if data is None:
            self.t.fill_(fill)
        else:
            self.t.copy_(torch.from_numpy(self.host.ravel()))
        assert self.t.data_ptr() % 16 == 4 * misalign, "the allocator's blocks are expected to be 16-byte aligned"

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def canaries_intact(self):
        return bool((self.buf[:self.front] == CANARY).all()) and bool((self.buf[self.front + self.n:] == CANARY).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.uint32), self.host.ravel().view(np.uint32))


def _same_bits(a, b):
    return torch.equal(a.t.view(torch.int32), b.t.view(torch.int32))


def _last_path():
    f, b = C.c_int32(-1), C.c_int32(-1)
    _lib.check(_lib.lib().pk2_lstm_last_path(C.byref(f), C.byref(b)))
    return f.value, b.value


class Run:
    """One case on the device.  Collects everything that is wrong and fails once, at the end, with all of it."""

    def __init__(self, case, label, regime, misalign=0):
        self.c, self.label, self.regime, self.mis = case, label, regime, misalign
        self.out = {}
        self.B, self.T, self.H, self.D = case["B"], case["T"], case["H"], case["D"]
        self.problems, self.ratios = [], {}
        self.L = _lib.lib()
        m = misalign
        # whh stays aligned: the host does not test it
        self.gx, self.whh = Guarded(case["gx"], misalign=m), Guarded(case["whh"])
        self.bhh = None if case["bhh"] is None else Guarded(case["bhh"], misalign=m)
        self.dy = Guarded(case["dy"], misalign=m)

    def note(self, what):
        self.problems.append("%s: %s" % (self.label, what))

    def check_guards(self, stage, **tensors):
        for name, g in tensors.items():
            if g is not None and not g.canaries_intact():
                self.note("%s: written outside %s" % (stage, name))

    def check_inputs(self, stage, **tensors):
        for name, g in tensors.items():
            if g is not None and not g.unchanged():
                self.note("%s: input %s was written" % (stage, name))

    def check_status(self, stage, fwd=None, bwd=None):
        f, b = _last_path()
        if fwd is not None and f != fwd:
            self.note("%s: forward path %s, expected %s" % (stage, PATH_NAME[f], PATH_NAME[fwd]))
        if bwd is not None and b != bwd:
            self.note("%s: backward path %s, expected %s" % (stage, PATH_NAME[b], PATH_NAME[bwd]))
        flag = C.c_uint32(7)
        _lib.check(self.L.pk2_lstm_persist_status(C.byref(flag)))
        if flag.value != 0:
            self.note("%s: a poll of a persistent recurrence timed out" % stage)
        if _lib.persist_guard_raised():
            self.note("%s: the guard of the persistent kernels is raised" % stage)

    def compare(self, stage, path, got, ref64, ref32):
        factors = {name: f for (p, name), f in FACTORS.items() if p == path}
        failures, ratios = lstm_check.compare(got, ref64, ref32, factors=factors)
        for _, msg in failures:
            self.note("%s [%s]: %s" % (stage, PATH_NAME[path], msg))
        for name, r in ratios.items():
            key = (stage, PATH_NAME[path], name)
            self.ratios[key] = max(self.ratios.get(key, 0.0), r)

    # ---- forward ------------------------------------------------------------------------------------------------------
    def forward_once(self, null_workspace=False):
        B, T, H, D = self.B, self.T, self.H, self.D
        m = self.mis
        y, gates, cells = Guarded(n=T * B * D * H, misalign=m), Guarded(n=D * T * B * 4 * H, misalign=m), Guarded(n=D * T * B * H, misalign=m)
        nws = int(self.L.pk2_lstm_fwd_workspace_floats(B, H, D))
        ws = Guarded(n=nws) if nws and not null_workspace else None
        _lib.check(self.L.pk2_lstm_layer_fwd(self.gx.ptr, self.whh.ptr, self.bhh.ptr if self.bhh else None, B, T, H, D, y.ptr,
                                             gates.ptr, cells.ptr, ws.ptr if ws else None, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return y, gates, cells, ws

    def forward(self, path, null_workspace=False):
        B, T, H, D = self.B, self.T, self.H, self.D
        y, gates, cells, ws = self.forward_once(null_workspace)
        self.check_status("forward", fwd=path)
        self.check_guards("forward", y=y, gates=gates, cells=cells, workspace=ws, gx=self.gx, whh=self.whh, bhh=self.bhh)
        self.check_inputs("forward", gx=self.gx, whh=self.whh, bhh=self.bhh)
        self.f64, self.f32 = lstm_check.forward_refs(self.c)
        self.dev = dict(y=y.numpy((T, B, D * H)), gates=gates.numpy((D, T, B, 4 * H)), cells=cells.numpy((D, T, B, H)))
        self.compare("forward", path, self.dev, self.f64, self.f32)
        y2, gates2, cells2, ws2 = self.forward_once(null_workspace)        # "a bit-reproducible forward pass"
        self.check_status("forward again", fwd=path)
        self.check_guards("forward again", y=y2, gates=gates2, cells=cells2, workspace=ws2)
        for name, a, b in (("y", y, y2), ("gates", gates, gates2), ("cells", cells, cells2)):
            if not _same_bits(a, b):
                self.note("forward [%s]: %s differs between two calls on the same inputs" % (PATH_NAME[path], name))

    # ---- backward -----------------------------------------------------------------------------------------------------
    def backward_once(self, gates, cells, with_bias_args, seed):
        B, T, H, D = self.B, self.T, self.H, self.D
        dgx = Guarded(n=T * B * D * 4 * H, misalign=self.mis)
        scratch = Guarded(n=int(self.L.pk2_lstm_bwd_scratch_floats(B, H, D)))
        r = np.random.default_rng(seed)
        # the accumulators: pre-filled with DIFFERENT random values
        b_ih, b_hh = Guarded(r.standard_normal((D, 4 * H))), Guarded(r.standard_normal((D, 4 * H)) * 3.0)
        done = C.c_int32(-1)
        if with_bias_args:
            _lib.check(self.L.pk2_lstm_layer_bwd_bias(self.dy.ptr, self.whh.ptr, gates.ptr, cells.ptr, B, T, H, D, dgx.ptr, scratch.ptr,
                                                      b_ih.ptr, b_hh.ptr, C.byref(done), _lib.stream_ptr()))
        else:
            _lib.check(self.L.pk2_lstm_layer_bwd(self.dy.ptr, self.whh.ptr, gates.ptr, cells.ptr, B, T, H, D, dgx.ptr, scratch.ptr,
                                                 _lib.stream_ptr()))
        torch.cuda.synchronize()
        return dgx, scratch, b_ih, b_hh, done.value

    def backward(self, path, gates_host, cells_host, stage, full):
        """Backward from the given float32 activations.  full: also the repeated call and the form without bias arguments."""
        B, T, H, D = self.B, self.T, self.H, self.D
        gates, cells = Guarded(gates_host, misalign=self.mis), Guarded(cells_host, misalign=self.mis)
        dgx, scratch, b_ih, b_hh, done = self.backward_once(gates, cells, True, seed=3)
        self.check_status(stage, bwd=path)
        self.check_guards(stage, dgx=dgx, scratch=scratch, dbias_ih=b_ih, dbias_hh=b_hh, dy=self.dy, gates=gates, cells=cells, whh=self.whh)
        self.check_inputs(stage, dy=self.dy, gates=gates, cells=cells, whh=self.whh)
        got = dict(dgx=dgx.numpy((T, B, D * 4 * H)))
        if done == 1:            # both accumulators have grown by the oracle's dbias
            got.update(dbias_ih=b_ih.numpy((D, 4 * H)), dbias_hh=b_hh.numpy((D, 4 * H)))
        elif done == 0:          # the path cannot fill them: both are bit-identical to what was put in
            if not (b_ih.unchanged() and b_hh.unchanged()):
                self.note("%s: *bias_done = 0 but the accumulators were written" % stage)
        else:
            self.note("%s: *bias_done = %d" % (stage, done))
        if (done == 1) != (path == SEQ):
            self.note("%s [%s]: *bias_done = %d (the bias gradients come out of lstm_bwd_seq2 only)" % (stage, PATH_NAME[path], done))
        r64, r32 = lstm_check.backward_refs(self.c, gates_host, cells_host, b_ih.host, b_hh.host)
        self.compare(stage, path, got, r64, r32)
        self.out[stage] = got
        if not full:
            return
        dgx2, scratch2, b_ih2, b_hh2, done2 = self.backward_once(gates, cells, True, seed=3)
        self.check_status(stage + " again", bwd=path)
        self.check_guards(stage + " again", dgx=dgx2, scratch=scratch2, dbias_ih=b_ih2, dbias_hh=b_hh2)
        if not _same_bits(dgx, dgx2):
            self.note("%s [%s]: dgx differs between two calls on the same inputs" % (stage, PATH_NAME[path]))
        if done2 != done:
            self.note("%s: *bias_done %d, then %d" % (stage, done, done2))
        atomics = path == SEQ and B > 1        # B atomicAdds per accumulator element, in the order the pairs finish
        if not atomics and not (_same_bits(b_ih, b_ih2) and _same_bits(b_hh, b_hh2)):
            self.note("%s [%s]: the bias gradients differ between two calls on the same inputs" % (stage, PATH_NAME[path]))
        dgx3, scratch3, b_ih3, b_hh3, _ = self.backward_once(gates, cells, False, seed=3)        # pk2_lstm_layer_bwd
        self.check_status(stage + ", pk2_lstm_layer_bwd", bwd=path)
        self.check_guards(stage + ", pk2_lstm_layer_bwd", dgx=dgx3, scratch=scratch3)
        if not _same_bits(dgx, dgx3):
            self.note("%s [%s]: pk2_lstm_layer_bwd and pk2_lstm_layer_bwd_bias give different dgx" % (stage, PATH_NAME[path]))
        if not (b_ih3.unchanged() and b_hh3.unchanged()):
            self.note("%s: memory the call was not given was written" % stage)

    def finish(self):
        for (stage, path, name), r in sorted(self.ratios.items()):
            print("lstm_layer_ratio | %s | %s | %s | %s | %s | %.3f" % (self.label, self.regime, stage, path, name, r))
        assert not self.problems, "\n".join(self.problems)


def _bwd_path(fwd_path):
    """The backward path of a case whose forward path is fwd_path: the same family; of the two backward forms of the
    large-batch family PK2_LSTM_BIG_BWD=1 (read once per process) selects the all-gather one."""
    if fwd_path == BIG and os.environ.get("PK2_LSTM_BIG_BWD") == "1":
        return BIG_AG
    return fwd_path


def run_case(B, T, H, D, regime, with_bias, path, forward_only=False, null_workspace=False):
    case = lstm_check.make_case(B, T, H, D, regime, with_bias, seed=1000 * B + 10 * T + D)
    run = Run(case, "B%d-T%d-H%d-D%d-%s" % (B, T, H, D, "bhh" if with_bias else "nobhh"), regime)
    run.forward(path, null_workspace)
    if not forward_only:
        # from the oracle's activations, so that a backward defect is not hidden behind, or blamed on, the forward pass
        run.backward(_bwd_path(path), run.f64["gates"].astype(np.float32), run.f64["cells"].astype(np.float32),
                     "backward from the oracle's activations", full=True)
        if np.isfinite(run.dev["gates"]).all() and np.isfinite(run.dev["cells"]).all():
            run.backward(_bwd_path(path), run.dev["gates"], run.dev["cells"], "backward from the device's activations", full=False)
    run.finish()
    return run


def _cases(cases):
    """(B, T, H, D) -> pytest params; every second case of a list passes bhh = NULL."""
    return [pytest.param(B, T, H, D, i % 2 == 0, id="B%d-T%d-H%d-D%d" % (B, T, H, D)) for i, (B, T, H, D) in enumerate(cases)]


REGIMES = pytest.mark.parametrize("regime", ["linear", "saturated"])

# 16 pairs: two teams per XCD; 32 pairs: the bound -- (32, 5, 1) has B >= 32 and still belongs to SEQ
SEQ_CASES = [(1, 1, 512, 1), (1, 2, 512, 2), (3, 65, 512, 2), (5, 130, 512, 1), (8, 9, 512, 2), (16, 8, 512, 2), (32, 5, 512, 1)]
STEP_SMALL_CASES = ([(17, 4, 512, 2)] +                    # 34 pairs: the first one past the bound of SEQ
                    [c for H in (64, 128, 256, 1024) for c in ((1, 1, H, 1), (5, 9, H, 2), (17, 65, H, 2), (31, 8, H, 1))] +
                    [(3, T, 128, 2) for T in (7, 8, 9, 63, 64, 72, 73)])      # graph tiers of 8 and 64 steps, overshoot skipped
STEP_SMALL_NO_SEQ_CASES = [(1, 1, 512, 1), (3, 65, 512, 2), (16, 8, 512, 2)]
# ragged last 64-row tiles; (2048, 1, 2): 64 tasks, the bound
BIG_CASES = [(32, 3, 512, 2), (33, 2, 512, 1), (64, 1, 512, 2), (65, 3, 512, 2), (129, 2, 512, 2), (2048, 1, 512, 2)]
STEP_BIG_CASES = ([(2049, 1, 512, 2)] +                    # 66 tasks: past the bound of BIG
                  [c for H in (64, 128, 256, 1024) for c in ((32, 2, H, 2), (33, 9, H, 1), (70, 8, H, 2), (64, 1, H, 1))])
STEP_BIG_NO_PERSIST_CASES = [(33, 6, 512, 1), (70, 9, 512, 2)]


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(SEQ_CASES))
def test_seq(B, T, H, D, with_bias, regime):
    run_case(B, T, H, D, regime, with_bias, SEQ)


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(STEP_SMALL_CASES))
def test_step_small(B, T, H, D, with_bias, regime):
    run_case(B, T, H, D, regime, with_bias, STEP_SMALL)


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(STEP_SMALL_NO_SEQ_CASES))
def test_step_small_without_seq(B, T, H, D, with_bias, regime, monkeypatch):
    monkeypatch.setenv("PK2_LSTM_SEQ", "0")
    run_case(B, T, H, D, regime, with_bias, STEP_SMALL)


@REGIMES
@pytest.mark.parametrize("with_bias", [True, False])
def test_step_small_forward_null_workspace(with_bias, regime):
    """pk2_lstm_layer_fwd with B >= 32 and workspace = NULL: the branch is meant (include/pk2hip.h; callers that hold no
    workspace, e.g. tools/ubench/side_stream_effect.py) -- lstm_fwd_step covers any batch in groups of 64 rows over
    grid.z -- and it is STEP_SMALL."""
    run_case(40, 3, 128, 2, regime, with_bias, STEP_SMALL, forward_only=True, null_workspace=True)


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(BIG_CASES))
def test_big(B, T, H, D, with_bias, regime):
    """Backward: lstm_bwd_big_persist2, or lstm_bwd_big_persist (BIG_AG) in a process started with PK2_LSTM_BIG_BWD=1."""
    run_case(B, T, H, D, regime, with_bias, BIG)


def test_big_all_gather_backward():
    """The cases of test_big in a fresh child process with PK2_LSTM_BIG_BWD=1 (the variable is read once per process):
    forward BIG, backward BIG_AG."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-x", "-k", "test_big and not all_gather"],
                         env=dict(os.environ, PK2_LSTM_BIG_BWD="1"), capture_output=True, text=True, timeout=600, cwd=root)
    print(out.stdout[-20000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert "%d passed" % (2 * len(BIG_CASES)) in out.stdout and "failed" not in out.stdout, out.stdout[-2000:]
    assert "| BIG_AG | dgx |" in out.stdout and "| BIG | dgx |" not in out.stdout


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(STEP_BIG_CASES))
def test_step_big(B, T, H, D, with_bias, regime):
    run_case(B, T, H, D, regime, with_bias, STEP_BIG)


@REGIMES
@pytest.mark.parametrize("B,T,H,D,with_bias", _cases(STEP_BIG_NO_PERSIST_CASES))
def test_step_big_without_persist(B, T, H, D, with_bias, regime, monkeypatch):
    """What a failed first-use check leaves the CE configuration with: the step kernels at H = 512."""
    monkeypatch.setenv("PK2_LSTM_BIG_PERSIST", "0")
    run_case(B, T, H, D, regime, with_bias, STEP_BIG)


@REGIMES
@pytest.mark.parametrize("with_bias", [True, False])
def test_unaligned_tensors_fall_back(with_bias, regime):
    """The tensors whose alignment the host tests (gx, y, gates, cells, bhh forward; dy, gates, cells, dgx backward) 4-byte
    but not 16-byte aligned at H = 512, B = 70: the forward pass keeps the step kernels (STEP_BIG), the backward pass the
    all-gather form (BIG_AG).  whh stays aligned (the host does not test it; every kernel moves it as 16-byte words).
    Read in the kernels before this was run: lstm_fwd_step_big and lstm_bwd_big_persist address gx, bhh, cells, gates, dy
    and every store by single floats; their only 16-byte accesses to these tensors are the loads of h_{t-1} (y, through
    gemm_tile.h's float4 slabs) and of the d gates of the step before (dgx) -- global_load_dwordx4 at a 4-byte-aligned
    address, which gfx950 serves (vector memory instructions need dword alignment; only LDS b128 needs 16 bytes)."""
    B, T, H, D = 70, 5, 512, 2
    case = lstm_check.make_case(B, T, H, D, regime, with_bias, seed=77)
    first = Run(case, "aligned-B70-T5-H512-D2", regime)       # verifies the family, whatever ran before in this process
    first.forward(BIG)
    first.finish()
    run = Run(case, "unaligned-B70-T5-H512-D2-%s" % ("bhh" if with_bias else "nobhh"), regime, misalign=1)
    run.forward(STEP_BIG)
    run.backward(BIG_AG, run.f64["gates"].astype(np.float32), run.f64["cells"].astype(np.float32),
                 "backward from the oracle's activations", full=True)
    if np.isfinite(run.dev["gates"]).all() and np.isfinite(run.dev["cells"]).all():
        run.backward(BIG_AG, run.dev["gates"], run.dev["cells"], "backward from the device's activations", full=False)
    run.finish()


def test_stale_graph_parameters():
    """Three cases that share the cached step graphs (same key: H, D, stream) with different B, T and pointers, fresh
    buffers each time: the third repeats the first and must give its bits."""
    runs = [run_case(B, T, 128, 2, "linear", True, STEP_SMALL) for B, T in ((5, 9), (3, 73), (5, 9))]
    for name in ("y", "gates", "cells"):
        assert np.array_equal(runs[0].dev[name].view(np.uint32), runs[2].dev[name].view(np.uint32)), name
    for stage in ("backward from the oracle's activations", "backward from the device's activations"):
        assert np.array_equal(runs[0].out[stage]["dgx"].view(np.uint32), runs[2].out[stage]["dgx"].view(np.uint32)), stage
