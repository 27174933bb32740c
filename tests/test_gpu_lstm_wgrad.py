"""The recurrent weight gradient from inside the small-batch backward recurrence (pk2_lstm_layer_bwd_wgrad, kernel
lstm_bwd_seq2_wgrad + lstm_seq_wgrad_reduce of csrc/lstm_persist_seq.hip) straight through the C ABI, against

    dwhh64[d] = dwhh_before[d] + sum_t sum_b dg64[t, b]^T h[t -+ 1, b]          (float64; d = 0: t - 1, d = 1: t + 1)

with dg64 the d gx of the float64 layer oracle (oracle/lstm_ref.py) and h the y the call is given.  The bound is the one of
tests/lstm_check.py, never taken from the kernel:

    max |dwhh_device - dwhh64|  <=  4 * max(e32, 2^-23 max |dwhh64|)

e32 = the error of the same sum from the float32 oracle's d gx, accumulated frame by frame in float32 per sequence (the
honest model of an accumulator that adds one frame at a time) and the sequences' sums added in ascending order.

Cases (H = 512 is the only size the kernel has): (1, 1, 1) no partner frame; (1, 2, 2) one product per direction -- the
time shift and its sign; (3, 5, 2) fewer pairs than teams, the prefetch ring wraps, the sum over sequences; (4, 19, 2) eight
pairs on eight XCDs, T past the 8-deep mail ring; (5, 7, 2) ten pairs: a team runs a second pair, the accumulators are
flushed and cleared between pairs; (8, 9, 2) two teams per XCD; (32, 5, 1) four pairs per team.

Which outcome a case must report.  Up to 8 pairs the launch has one team per XCD, one workgroup per CU, which any kernel
that can be launched at all has room for: done = 1 is required.  More than 8 pairs ask for two teams per XCD, two workgroups
per CU, and a workgroup holds its 64 x 512 slice of W_hh AND its 64 x 512 slice of dW_hh in registers -- 2 x 128 KB, two
workgroups the CU's whole 512 KB register file (the listing: 256 + 192 registers per lane, one workgroup per CU).  So for
(5, 7, 2), (8, 9, 2) and (32, 5, 1) done = 0 with dwhh and the workspace untouched is as legal as done = 1 with a correct
sum, whichever is reported is asserted (the MI355X reports 0), and the same three cases run again with
PK2_LSTM_SEQ_WGRAD=2 -- one team per XCD where two are not resident -- where done = 1 is required: that is where a team
runs a second pair (ten pairs on eight teams), two (16 pairs) and four pairs (32 pairs) and flushes and clears its
accumulators between them.

Measured on the MI355X, error / max(e32, floor) of dwhh per case (linear / saturated): (1, 1, 1) 0 / 0; (1, 2, 2) 0.43 /
0.51; (3, 5, 2) 0.68 / 0.92; (4, 19, 2) 1.07 / 1.00; with one team per XCD (5, 7, 2) 0.81 / 0.55; (8, 9, 2) 0.90 / 1.16;
(32, 5, 1) 1.02 / 0.96 (profiles/wgrad_in_recurrence.txt).  No case needs more than the common factor 4: the f32 MFMA is
an fma chain per frame, which is what e32 models.

Every case also: dwhh pre-filled with non-zero values (+=), guard bands around dwhh and the workspace (a full-sized one in
every call, also where the library asks for none because it will not fuse: "untouched" is checked on memory), the inputs
bit-unchanged, d gx bit-identical to pk2_lstm_layer_bwd_bias, the bias gradients within the layer file's bound, no poll
timed out, the guard not raised, dwhh bit-identical over two calls (the sum's order is fixed by construction: MFMA
accumulators per pair, the pairs' slices added b = 0 .. B - 1 by one thread per element -- no float atomics).  No test
provokes a timeout: that lstm_seq_wgrad_reduce writes NaN after a launch that gave up (the sticky word seq_exit_check
sets before the reduction starts) is established by reading it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bound_check
import lstm_check
from pykaldi2_amd import _lib
from test_gpu_lstm_layer import Guarded, _last_path, _same_bits, SEQ

pytestmark = pytest.mark.gpu

H = 512
WS_FILL = 7.25
# (B, T, D): must the fused kernel have run?  (False: either outcome is legal, see above)
CASES = [(B, T, D, B * D <= 8) for B, T, D in [(1, 1, 1), (1, 2, 2), (3, 5, 2), (4, 19, 2), (5, 7, 2), (8, 9, 2), (32, 5, 1)]]
CASES += [(B, T, D, "one team") for B, T, D, must in CASES if not must]


def dwhh_refs(y, dgx64, dgx32, dwhh0, B, T, D):
    """(float64 reference, float32 frame-by-frame model) of dwhh after the call, [D][4H][H]."""
    G = 4 * H
    want = dwhh0.astype(np.float64).copy()
    model = np.zeros((D, G, H), np.float32)
    for d in range(D):
        dg64, dg32, h = dgx64[:, :, d * G:(d + 1) * G], dgx32[:, :, d * G:(d + 1) * G].astype(np.float32), y[:, :, d * H:(d + 1) * H]
        if T > 1:
            a, b = (slice(1, T), slice(0, T - 1)) if d == 0 else (slice(0, T - 1), slice(1, T))     # dg[t] with h[t - 1] / h[t + 1]
            want[d] += np.einsum("tbr,tbk->rk", dg64[a], h[b].astype(np.float64))
        for s in range(B):
            acc = np.zeros((G, H), np.float32)
            order = range(T - 1, 0, -1) if d == 0 else range(0, T - 1)       # the frames in the order the backward pass visits them
            for t in order:
                acc += np.outer(dg32[t, s], h[t - 1 if d == 0 else t + 1, s])
            model[d] = acc if s == 0 else model[d] + acc
    return want, (dwhh0 + model).astype(np.float32)


class Case:
    """One case's data and references, computed once and shared by the tests that need it (read-only)."""
    _cache = {}

    @classmethod
    def get(cls, B, T, D, regime):
        key = (B, T, D, regime)
        if key not in cls._cache:
            cls._cache[key] = cls(B, T, D, regime)
        return cls._cache[key]

    def __init__(self, B, T, D, regime):
        self.B, self.T, self.D, self.regime = B, T, D, regime
        self.c = lstm_check.make_case(B, T, H, D, regime, True, seed=7000 + 1000 * B + 10 * T + D)
        f64, _ = lstm_check.forward_refs(self.c)
        # the forward pass's tensors as float32, from the oracle: a backward defect is not blamed on the forward pass
        self.y, self.gates, self.cells = (f64[k].astype(np.float32) for k in ("y", "gates", "cells"))
        r = np.random.default_rng(11 + B)
        self.b_ih0, self.b_hh0 = r.standard_normal((D, 4 * H)).astype(np.float32), (3.0 * r.standard_normal((D, 4 * H))).astype(np.float32)
        self.dwhh0 = (0.5 + r.random((D, 4 * H, H))).astype(np.float32) * np.where(r.random((D, 4 * H, H)) < 0.5, -1.0, 1.0).astype(np.float32)
        self.r64, self.r32 = lstm_check.backward_refs(self.c, self.gates, self.cells, self.b_ih0, self.b_hh0)
        self.dwhh64, self.dwhh32 = dwhh_refs(self.y, self.r64["dgx"], self.r32["dgx"], self.dwhh0, B, T, D)


class Call:
    """One pk2_lstm_layer_bwd_wgrad (or _bwd_bias) call on fresh guarded buffers."""

    def __init__(self, k, dev, wgrad=True):
        L = _lib.lib()
        B, T, D = k.B, k.T, k.D
        self.dgx = Guarded(n=T * B * D * 4 * H)
        self.scratch = Guarded(n=int(L.pk2_lstm_bwd_scratch_floats(B, H, D)))
        self.b_ih, self.b_hh, self.dwhh = Guarded(k.b_ih0), Guarded(k.b_hh0), Guarded(k.dwhh0)
        # (where the library asks for no workspace, because it will not fuse, it gets a full-sized one all the same: "the
        # workspace is untouched" is then a check of memory that exists)
        self.nws_asked = int(L.pk2_lstm_bwd_wgrad_workspace_floats(B, H, D))
        assert self.nws_asked in (0, B * D * 4 * H * H), self.nws_asked
        self.ws = Guarded(n=B * D * 4 * H * H, fill=WS_FILL)
        bias_done, whh_done = C.c_int32(-1), C.c_int32(-1)
        if wgrad:
            _lib.check(L.pk2_lstm_layer_bwd_wgrad(dev["dy"].ptr, dev["whh"].ptr, dev["gates"].ptr, dev["cells"].ptr, dev["y"].ptr, B, T, H, D,
                                                  self.dgx.ptr, self.scratch.ptr, self.b_ih.ptr, self.b_hh.ptr, self.dwhh.ptr,
                                                  self.ws.ptr, C.byref(bias_done), C.byref(whh_done), _lib.stream_ptr()))
        else:
            _lib.check(L.pk2_lstm_layer_bwd_bias(dev["dy"].ptr, dev["whh"].ptr, dev["gates"].ptr, dev["cells"].ptr, B, T, H, D, self.dgx.ptr,
                                                 self.scratch.ptr, self.b_ih.ptr, self.b_hh.ptr, C.byref(bias_done), _lib.stream_ptr()))
        torch.cuda.synchronize()
        self.bias_done, self.whh_done = bias_done.value, whh_done.value

    def ws_untouched(self):
        return bool((self.ws.t == WS_FILL).all())


def on_device(k):
    """The case's inputs on the device, and one forward call (a backward call before a verified forward one keeps the
    step kernels)."""
    L = _lib.lib()
    B, T, D = k.B, k.T, k.D
    dev = dict(dy=Guarded(k.c["dy"]), whh=Guarded(k.c["whh"]), gates=Guarded(k.gates), cells=Guarded(k.cells), y=Guarded(k.y))
    gx, bhh = Guarded(k.c["gx"]), Guarded(k.c["bhh"])
    y, gates, cells = Guarded(n=T * B * D * H), Guarded(n=D * T * B * 4 * H), Guarded(n=D * T * B * H)
    _lib.check(L.pk2_lstm_layer_fwd(gx.ptr, dev["whh"].ptr, bhh.ptr, B, T, H, D, y.ptr, gates.ptr, cells.ptr, None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dev


def clean_status(problems, stage):
    flag = C.c_uint32(7)
    _lib.check(_lib.lib().pk2_lstm_persist_status(C.byref(flag)))
    if flag.value != 0:
        problems.append("%s: a poll of a persistent recurrence timed out" % stage)
    if _lib.persist_guard_raised():
        problems.append("%s: the guard of the persistent kernels is raised" % stage)
    if _last_path()[1] != SEQ:
        problems.append("%s: backward path %d, expected SEQ" % (stage, _last_path()[1]))


def check_call(k, dev, call, stage, problems):
    """Everything a call is held to but the value of dwhh when done."""
    clean_status(problems, stage)
    for name, g in dict(dgx=call.dgx, scratch=call.scratch, dbias_ih=call.b_ih, dbias_hh=call.b_hh, dwhh=call.dwhh, wgrad_ws=call.ws, **dev).items():
        if g is not None and not g.canaries_intact():
            problems.append("%s: written outside %s" % (stage, name))
    for name, g in dev.items():
        if not g.unchanged():
            problems.append("%s: input %s was written" % (stage, name))
    if call.bias_done != 1:
        problems.append("%s: *bias_done = %d" % (stage, call.bias_done))
    got = dict(dgx=call.dgx.numpy((k.T, k.B, k.D * 4 * H)), dbias_ih=call.b_ih.numpy((k.D, 4 * H)), dbias_hh=call.b_hh.numpy((k.D, 4 * H)))
    failures, ratios = lstm_check.compare(got, k.r64, k.r32)
    problems += ["%s: %s" % (stage, msg) for _, msg in failures]
    return ratios


@pytest.mark.parametrize("regime", ["linear", "saturated"])
@pytest.mark.parametrize("B,T,D,must_fuse", [pytest.param(*c, id="B%d-T%d-D%d%s" % (c[:3] + ("-one-team" if c[3] == "one team" else "",))) for c in CASES])
def test_wgrad(B, T, D, must_fuse, regime, monkeypatch):
    if must_fuse == "one team":
        monkeypatch.setenv("PK2_LSTM_SEQ_WGRAD", "2")
    k = Case.get(B, T, D, regime)
    dev = on_device(k)
    problems = []
    first = Call(k, dev)
    check_call(k, dev, first, "first call", problems)
    plain = Call(k, dev, wgrad=False)                  # pk2_lstm_layer_bwd_bias on the same inputs
    if not _same_bits(first.dgx, plain.dgx):
        problems.append("dgx differs from pk2_lstm_layer_bwd_bias")
    if first.whh_done not in (0, 1) or (must_fuse and first.whh_done != 1):
        problems.append("*whh_done = %d" % first.whh_done)
    if first.whh_done == 1:
        got = first.dwhh.numpy((D, 4 * H, H))
        if T == 1:
            if not first.dwhh.unchanged():
                problems.append("T = 1: dwhh was changed")
            if not first.ws_untouched():
                problems.append("T = 1: the workspace was written")
        failures, ratios = bound_check.compare(dict(dwhh=got), dict(dwhh=k.dwhh64), dict(dwhh=k.dwhh32), ("dwhh",))
        print("lstm_wgrad_ratio | B%d-T%d-D%d | %s | %s | dwhh | %.3f" % (B, T, D, regime, must_fuse, ratios["dwhh"]))
        problems += [msg for _, msg in failures]
        second = Call(k, dev)
        check_call(k, dev, second, "second call", problems)
        if second.whh_done != 1:
            problems.append("*whh_done = 1, then %d" % second.whh_done)
        if not _same_bits(first.dwhh, second.dwhh):
            problems.append("dwhh differs between two calls on the same inputs")
    else:
        print("lstm_wgrad_ratio | B%d-T%d-D%d | %s | dwhh | not done" % (B, T, D, regime))
        if not first.dwhh.unchanged():
            problems.append("*whh_done = 0 but dwhh was written")
        if not first.ws_untouched():
            problems.append("*whh_done = 0 but the workspace was written")
    assert not problems, "\n".join(problems)


def test_wgrad_switched_off(monkeypatch):
    """PK2_LSTM_SEQ_WGRAD=0 (read per call): done = 0, nothing written, the recurrence as before."""
    k = Case.get(3, 5, 2, "linear")
    dev = on_device(k)
    problems = []
    on = Call(k, dev)
    monkeypatch.setenv("PK2_LSTM_SEQ_WGRAD", "0")
    off = Call(k, dev)
    check_call(k, dev, off, "switched off", problems)
    assert on.whh_done == 1 and off.whh_done == 0, (on.whh_done, off.whh_done)
    assert on.nws_asked == k.B * k.D * 4 * H * H and off.nws_asked == 0, (on.nws_asked, off.nws_asked)
    assert not on.ws_untouched()                       # (the check below can tell a written workspace from an unwritten one)
    assert off.dwhh.unchanged() and off.ws_untouched()
    assert _same_bits(on.dgx, off.dgx)
    assert not problems, "\n".join(problems)


def test_model_gradients_with_and_without(monkeypatch):
    """LSTMAM, one bidirectional layer, B = 3, T = 11: every parameter gradient with the fusion on and off agrees within the
    sum of the two paths' bounds against torch's float64 CPU LSTM (bound of a path: 4 * max(e32, floor), e32 from torch's
    float32 CPU LSTM on the same data)."""
    from pykaldi2_amd import lstm
    torch.manual_seed(311)
    B, T, Din, P = 3, 11, 40, 24
    m = lstm.LSTMAM(Din, P, H, 1, 0.0, True)
    x, wgt = torch.randn(B, T, Din), torch.randn(B, T, P)
    refs = []
    for dt in (torch.float64, torch.float32):
        ref_lstm = torch.nn.LSTM(Din, H, 1, batch_first=True, bidirectional=True).to(dt)
        ref_out = torch.nn.Linear(2 * H, P).to(dt)
        ref_lstm.load_state_dict({n[5:]: v.to(dt) for n, v in m.state_dict().items() if n.startswith("lstm.")})
        ref_out.load_state_dict({n[13:]: v.to(dt) for n, v in m.state_dict().items() if n.startswith("output_layer.")})
        (ref_out(ref_lstm(x.to(dt))[0]) * wgt.to(dt)).sum().backward()
        refs.append(dict([("lstm." + n, v.grad.numpy()) for n, v in ref_lstm.named_parameters()] +
                         [("output_layer." + n, v.grad.numpy()) for n, v in ref_out.named_parameters()]))
    m = m.cuda()
    # what the model's backward pass hands the entry and what the entry reports: with the switch on the recurrence must have
    # produced dW_hh (else on and off are the same computation and agree trivially), with it off the caller's product
    L, calls = _lib.lib(), []
    entry = L.pk2_lstm_layer_bwd_wgrad

    def recording_entry(*a):
        rc = entry(*a)
        calls.append(dict(y=a[4], dwhh=a[13], ws=a[14], whh_done=a[16]._obj.value))
        return rc

    monkeypatch.setattr(L, "pk2_lstm_layer_bwd_wgrad", recording_entry)
    grads = []
    for switch in ("1", "0"):
        monkeypatch.setenv("PK2_LSTM_SEQ_WGRAD", switch)
        m.zero_grad()
        (m(x.cuda()) * wgt.cuda()).sum().backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()})
    assert [c["whh_done"] for c in calls] == [1, 0], calls
    assert all(c["y"] and c["dwhh"] for c in calls) and calls[0]["ws"] and not calls[1]["ws"], calls
    flag = C.c_uint32(7)
    assert _lib.lib().pk2_lstm_persist_status(C.byref(flag)) == 0 and flag.value == 0 and not _lib.persist_guard_raised()
    assert _last_path() == (SEQ, SEQ)
    problems = []
    for name in refs[0]:
        unit, _, _ = bound_check.unit(refs[0][name], refs[1][name])
        diff = float(np.abs(grads[0][name].astype(np.float64) - grads[1][name]).max())
        print("lstm_wgrad_model | %s | on-off %.3g | bound %.3g | on/f64 %.3f | off/f64 %.3f" % (
            name, diff, 2 * bound_check.FACTOR * unit, float(np.abs(grads[0][name] - refs[0][name]).max()) / unit,
            float(np.abs(grads[1][name] - refs[0][name]).max()) / unit))
        if not (np.isfinite(grads[0][name]).all() and np.isfinite(grads[1][name]).all()):
            problems.append("%s: not finite" % name)
        elif not diff <= 2 * bound_check.FACTOR * unit:
            problems.append("%s: on and off differ by %.3g > %.3g" % (name, diff, 2 * bound_check.FACTOR * unit))
    assert not problems, "\n".join(problems)
