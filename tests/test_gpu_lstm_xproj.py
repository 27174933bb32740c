"""The input projections from inside the small-batch forward recurrence (pk2_lstm_layer_fwd_xproj, kernel
lstm_fwd_seq2_xproj of csrc/lstm_persist_seq.hip) straight through the C ABI, against the float64 layer oracle
(oracle/lstm_ref.py) run on

    gx64 = inp W_ih^T + b_ih                                        (float64)

The bound is the one of tests/lstm_check.py at its FACTOR, the same the unfused recurrence is held to, never taken from the
kernel: e32 comes from the float32 oracle run on the float32 product of the same data (numpy's).

Data.  whh, bhh as lstm_check.make_case makes them; inp ~ N(0, 1), W_ih ~ N(0, 1 / in_size), b_ih ~ U(+-1 / sqrt(H)), so gx is
N(0, 1) as in make_case's "linear" regime; "saturated": W_ih times 8 and 1 % of b_ih replaced by +-U(40, 120), make_case's
saturated gx produced by the operands (gates at exactly 0 and 1, exp2 overflowing inside both nonlinearities).

Cases (H = 512, in_size 80 and 1024): (1, 1, 1), (1, 2, 2), (2, 3, 2) the prologue and the clamped row pointers; (3, 5, 2);
(4, 31, 2), (4, 33, 2), (4, 65, 2) the boundaries of the blocks of 32 steps; (5, 7, 2), (8, 9, 2) more than 8 pairs: with the
switch at its default they must report gx_done = 0 and write nothing, with PK2_LSTM_SEQ_XPROJ=2 they must fuse and match --
that is where a team runs a second pair and starts its ring again.

Every fused call also: guard bands around every tensor, the inputs bit-unchanged, no poll timed out, the guard not raised,
the forward path reported SEQ, and the same bits over two calls (every sum's order is fixed by construction).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bound_check
import lstm_check
from oracle import lstm_ref
from pykaldi2_amd import _lib
from test_gpu_lstm_layer import Guarded, _last_path, _same_bits, SEQ

pytestmark = pytest.mark.gpu

H = 512
FILL = 7.25
SHAPES = [(1, 1, 1), (1, 2, 2), (2, 3, 2), (3, 5, 2), (4, 31, 2), (4, 33, 2), (4, 65, 2), (5, 7, 2), (8, 9, 2)]
# (B, T, D, switch, must the call fuse?)
CASES = [(B, T, D, "1", B * D <= 8) for B, T, D in SHAPES] + [(B, T, D, "2", True) for B, T, D in SHAPES if B * D > 8]


class Case:
    """One case's data and references, computed once and shared by the tests that need it (read-only)."""
    _cache = {}

    @classmethod
    def get(cls, B, T, D, K, regime):
        key = (B, T, D, K, regime)
        if key not in cls._cache:
            cls._cache[key] = cls(B, T, D, K, regime)
        return cls._cache[key]

    def __init__(self, B, T, D, K, regime):
        self.B, self.T, self.D, self.K, self.regime = B, T, D, K, regime
        c = lstm_check.make_case(B, T, H, D, regime, True, seed=9000 + 1000 * B + 10 * T + D + K)
        self.whh, self.bhh = c["whh"], c["bhh"]
        r = np.random.default_rng(77 + 1000 * B + 10 * T + D + K)
        self.inp = r.standard_normal((T, B, K)).astype(np.float32)
        w = r.standard_normal((D * 4 * H, K)) / np.sqrt(K)
        b = r.uniform(-1.0, 1.0, D * 4 * H) / np.sqrt(H)
        if regime == "saturated":
            w *= 8.0
            m = r.random(b.shape) < 0.01
            b[m] = np.where(r.random(int(m.sum())) < 0.5, -1.0, 1.0) * r.uniform(40.0, 120.0, int(m.sum()))
        self.w_ih, self.b_ih = w.astype(np.float32), b.astype(np.float32)
        gx64 = self.inp.astype(np.float64) @ self.w_ih.astype(np.float64).T + self.b_ih.astype(np.float64)
        self.gx32 = (self.inp @ self.w_ih.T + self.b_ih).astype(np.float32)
        self.r64 = dict(zip(("y", "gates", "cells"), lstm_ref.layer_fwd(gx64, self.whh, self.bhh, np.float64)))
        self.r32 = dict(zip(("y", "gates", "cells"), lstm_ref.layer_fwd(self.gx32, self.whh, self.bhh, np.float32)))


@pytest.fixture(scope="module", autouse=True)
def verified_device():
    """The first forward launch on a device is the one the host verifies; it is never fused.  One plain call first."""
    c = lstm_check.make_case(1, 2, H, 1, "linear", True, seed=1)
    gx, whh, bhh = Guarded(c["gx"]), Guarded(c["whh"]), Guarded(c["bhh"])
    y, gates, cells = Guarded(n=2 * H), Guarded(n=2 * 4 * H), Guarded(n=2 * H)
    _lib.check(_lib.lib().pk2_lstm_layer_fwd(gx.ptr, whh.ptr, bhh.ptr, 1, 2, H, 1, y.ptr, gates.ptr, cells.ptr, None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert _last_path()[0] == SEQ


def on_device(k):
    return dict(inp=Guarded(k.inp), w_ih=Guarded(k.w_ih), b_ih=Guarded(k.b_ih), whh=Guarded(k.whh), bhh=Guarded(k.bhh))


class Call:
    """One pk2_lstm_layer_fwd_xproj call on fresh guarded outputs (gx = NULL)."""

    def __init__(self, k, dev, in_size=None):
        B, T, D = k.B, k.T, k.D
        self.y, self.gates, self.cells = Guarded(n=T * B * D * H, fill=FILL), Guarded(n=D * T * B * 4 * H, fill=FILL), Guarded(n=D * T * B * H, fill=FILL)
        done = C.c_int32(-1)
        _lib.check(_lib.lib().pk2_lstm_layer_fwd_xproj(None, dev["whh"].ptr, dev["bhh"].ptr, B, T, H, D, self.y.ptr, self.gates.ptr,
                                                       self.cells.ptr, None, dev["inp"].ptr, k.K if in_size is None else in_size,
                                                       dev["w_ih"].ptr, dev["b_ih"].ptr, C.byref(done), _lib.stream_ptr()))
        torch.cuda.synchronize()
        self.done = done.value

    def outputs(self):
        return dict(y=self.y, gates=self.gates, cells=self.cells)

    def untouched(self):
        return all(bool((g.t == FILL).all()) for g in self.outputs().values())


def check_call(k, dev, call, stage, problems):
    flag = C.c_uint32(7)
    _lib.check(_lib.lib().pk2_lstm_persist_status(C.byref(flag)))
    if flag.value != 0:
        problems.append("%s: a poll of a persistent recurrence timed out" % stage)
    if _lib.persist_guard_raised():
        problems.append("%s: the guard of the persistent kernels is raised" % stage)
    for name, g in dict(call.outputs(), **dev).items():
        if not g.canaries_intact():
            problems.append("%s: written outside %s" % (stage, name))
    for name, g in dev.items():
        if not g.unchanged():
            problems.append("%s: input %s was written" % (stage, name))


@pytest.mark.parametrize("regime", ["linear", "saturated"])
@pytest.mark.parametrize("K", [80, 1024])
@pytest.mark.parametrize("B,T,D,switch,must_fuse", [pytest.param(*c, id="B%d-T%d-D%d-switch%s" % c[:4]) for c in CASES])
def test_xproj(B, T, D, switch, must_fuse, K, regime, monkeypatch):
    monkeypatch.setenv("PK2_LSTM_SEQ_XPROJ", switch)
    k = Case.get(B, T, D, K, regime)
    dev = on_device(k)
    problems = []
    first = Call(k, dev)
    check_call(k, dev, first, "first call", problems)
    if not must_fuse:
        assert first.done == 0 and first.untouched(), (first.done, first.untouched())
        assert not problems, "\n".join(problems)
        return
    assert first.done == 1, first.done
    if _last_path()[0] != SEQ:
        problems.append("forward path %d, expected SEQ" % _last_path()[0])
    got = dict(y=first.y.numpy((T, B, D * H)), gates=first.gates.numpy((D, T, B, 4 * H)), cells=first.cells.numpy((D, T, B, H)))
    failures, ratios = lstm_check.compare(got, k.r64, k.r32)
    for name in ("y", "gates", "cells"):
        print("lstm_xproj_ratio | B%d-T%d-D%d | K%d | %s | switch %s | %s | %.3f" % (B, T, D, K, regime, switch, name, ratios[name]))
    problems += [msg for _, msg in failures]
    second = Call(k, dev)
    check_call(k, dev, second, "second call", problems)
    if second.done != 1:
        problems.append("*gx_done = 1, then %d" % second.done)
    for name in ("y", "gates", "cells"):
        if not _same_bits(first.outputs()[name], second.outputs()[name]):
            problems.append("%s differs between two calls on the same inputs" % name)
    assert not problems, "\n".join(problems)


def test_unsupported_in_size_is_not_fused():
    """in_size = 96 (the operands of the K = 1024 case read with a row length of 96): gx_done = 0, nothing written."""
    k = Case.get(3, 5, 2, 1024, "linear")
    dev = on_device(k)
    problems = []
    call = Call(k, dev, in_size=96)
    check_call(k, dev, call, "in_size 96", problems)
    assert call.done == 0 and call.untouched(), (call.done, call.untouched())
    assert not problems, "\n".join(problems)


def test_switched_off(monkeypatch):
    """PK2_LSTM_SEQ_XPROJ=0 (read per call): gx_done = 0, nothing written, pk2_lstm_last_path reports what it reported."""
    k = Case.get(3, 5, 2, 80, "linear")
    dev = on_device(k)
    problems = []
    on = Call(k, dev)
    before = _last_path()
    monkeypatch.setenv("PK2_LSTM_SEQ_XPROJ", "0")
    off = Call(k, dev)
    check_call(k, dev, off, "switched off", problems)
    assert on.done == 1 and not on.untouched()
    assert off.done == 0 and off.untouched(), (off.done, off.untouched())
    assert _last_path() == before
    assert not problems, "\n".join(problems)


def test_model_with_and_without(monkeypatch):
    """LSTMAM(80, 97, 512, 3, 0.0, True), B = 3, T = 19, forward and backward with the switch at 0 and at 1: logits and every
    parameter gradient of the two runs agree within the sum of the two paths' bounds against torch's float64 CPU LSTM (bound
    of a path: 4 * max(e32, floor), e32 from torch's float32 CPU LSTM on the same data) -- the bound of
    test_gpu_lstm_wgrad.py::test_model_gradients_with_and_without."""
    from pykaldi2_amd import lstm
    torch.manual_seed(523)
    B, T, Din, P, Lr = 3, 19, 80, 97, 3
    m = lstm.LSTMAM(Din, P, H, Lr, 0.0, True)
    x, wgt = torch.randn(B, T, Din), torch.randn(B, T, P)
    refs = []
    for dt in (torch.float64, torch.float32):
        ref_lstm = torch.nn.LSTM(Din, H, Lr, batch_first=True, bidirectional=True).to(dt)
        ref_out = torch.nn.Linear(2 * H, P).to(dt)
        ref_lstm.load_state_dict({n[5:]: v.to(dt) for n, v in m.state_dict().items() if n.startswith("lstm.")})
        ref_out.load_state_dict({n[13:]: v.to(dt) for n, v in m.state_dict().items() if n.startswith("output_layer.")})
        logits = ref_out(ref_lstm(x.to(dt))[0])
        (logits * wgt.to(dt)).sum().backward()
        refs.append(dict([("lstm." + n, v.grad.numpy()) for n, v in ref_lstm.named_parameters()] +
                         [("output_layer." + n, v.grad.numpy()) for n, v in ref_out.named_parameters()] +
                         [("logits", logits.detach().numpy())]))
    m = m.cuda()
    L, calls = _lib.lib(), []
    entry = L.pk2_lstm_layer_fwd_xproj

    def recording_entry(*a):
        rc = entry(*a)
        calls.append(a[15]._obj.value)
        return rc

    monkeypatch.setattr(L, "pk2_lstm_layer_fwd_xproj", recording_entry)
    runs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("PK2_LSTM_SEQ_XPROJ", switch)
        m.zero_grad()
        logits = m(x.cuda())
        (logits * wgt.cuda()).sum().backward()
        torch.cuda.synchronize()
        run = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
        run["logits"] = logits.detach().cpu().numpy().copy()
        runs.append(run)
    assert calls == [1] * Lr + [0] * Lr, calls        # on: every layer multiplied inside its recurrence; off: none did
    flag = C.c_uint32(7)
    assert _lib.lib().pk2_lstm_persist_status(C.byref(flag)) == 0 and flag.value == 0 and not _lib.persist_guard_raised()
    assert _last_path() == (SEQ, SEQ)
    problems = []
    for name in refs[0]:
        unit, _, _ = bound_check.unit(refs[0][name], refs[1][name])
        diff = float(np.abs(runs[0][name].astype(np.float64) - runs[1][name]).max())
        print("lstm_xproj_model | %s | on-off %.3g | bound %.3g | on/f64 %.3f | off/f64 %.3f" % (
            name, diff, 2 * bound_check.FACTOR * unit, float(np.abs(runs[0][name] - refs[0][name]).max()) / unit,
            float(np.abs(runs[1][name] - refs[0][name]).max()) / unit))
        if not (np.isfinite(runs[0][name]).all() and np.isfinite(runs[1][name]).all()):
            problems.append("%s: not finite" % name)
        elif not diff <= 2 * bound_check.FACTOR * unit:
            problems.append("%s: on and off differ by %.3g > %.3g" % (name, diff, 2 * bound_check.FACTOR * unit))
    assert not problems, "\n".join(problems)
