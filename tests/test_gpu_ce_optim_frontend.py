"""csrc/softmax_ce.hip, csrc/optim.hip and csrc/fbank.hip through the C ABI (and through ops.CrossEntropyLoss, optim.*, fbank.*
where the Python wrapper adds logic) against the float64 oracles oracle/ce_ref.py, optim_ref.py and frontend_ref.logfbank64,
at the shapes where these kernels take another path: both CE variants and both of the streaming variant's triggers, rows that
a workgroup walks, row strides, every scale kernel on its float4 and its scalar path, Adam / SGD with every switch, the
grid-stride loops and the n % 4 tail of the norm, the per-32-utterance launches of the front end, the CMN partition tails and
the grid caps of the subsampling and normalisation kernels.

Every output sits in a buffer that is NaN where the kernel must write and SENTINEL around it and in stride gaps; the bands must
come back untouched.  Every input is surrounded by NaN, and stride gaps of an input hold NaN: a read outside shows in the result.
Inputs and bounds: tests/edge_cases.py; the float32 CPU models behind the bounds: tests/test_oracle_ce_optim.py.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import edge_cases as E
from oracle import ce_ref, frontend_ref as F, optim_ref
from pykaldi2_amd import _lib, fbank, ops, optim

pytestmark = pytest.mark.gpu

BAND = 64                 # floats of guard band on either side (a multiple of 4: the logical window stays 16-byte aligned)
S = np.float32(E.SENTINEL)


def L():
    return _lib.lib()


def sp():
    return _lib.stream_ptr()


class Buf:
    """A device buffer: `band` elements of `band_fill`, the logical array `host`, `band` elements again.  .ptr is the address
    of the logical array's first element (+ `off` elements: a base that is not 16-byte aligned), .t the logical window."""

    def __init__(self, host, band_fill, off=0):
        host = np.ascontiguousarray(host)
        self.n, self.lo = host.size, BAND + off
        full = np.full(self.n + 2 * BAND + off, band_fill, dtype=host.dtype)
        full[self.lo:self.lo + self.n] = host.reshape(-1)
        self.band_fill, self.shape = full[0].copy(), host.shape
        self.full = torch.from_numpy(full).cuda()
        self.t = self.full[self.lo:self.lo + self.n]
        self.ptr = ctypes.c_void_p(self.t.data_ptr())

    def host(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def bands_intact(self):
        h = self.full.cpu().numpy()
        edges = np.concatenate([h[:self.lo], h[self.lo + self.n:]])
        return bool(np.isnan(edges).all() if np.isnan(self.band_fill) else (edges == self.band_fill).all())


def out_f32(shape, off=0):
    """An output: NaN where the kernel must write, SENTINEL bands."""
    return Buf(np.full(shape, np.nan, np.float32), S, off)


def in_f32(host, off=0):
    """An input: NaN bands."""
    return Buf(np.asarray(host, np.float32), np.float32(np.nan), off)


# ================================================================================================================ softmax-CE
def run_ce(x, t, mean, row_stride=None, grad_stride=None, want_grad=True, want_lp=False, acc=None):
    """One call of pk2_softmax_ce_fwd_bwd (_mean) on logits x [rows, P] placed at row_stride with NaN gaps.  Returns
    dict(loss, count, grad [rows, P] or None, lp [rows, P] or None, acc)."""
    rows, P = x.shape
    rs, gs_ = row_stride or P, grad_stride or P
    xin = np.full((rows, rs), np.nan, np.float32)
    xin[:, :P] = x
    xb = in_f32(xin)
    tb = Buf(np.asarray(t, np.int64), np.int64(-100))
    if acc is None:                                   # the accumulators start as garbage: they are zeroed inside
        acc = (Buf(np.full(1, np.nan, np.float32), S), Buf(np.full(1, 77, np.int32), np.int32(-12345)))
    gb = lb = None
    if want_grad:
        g0 = np.full((rows, gs_), S, np.float32)
        g0[:, :P] = np.nan
        gb = Buf(g0, S)
    if want_lp:
        lb = out_f32((rows, P))
    if mean:
        assert want_grad and not want_lp
        _lib.check(L().pk2_softmax_ce_fwd_bwd_mean(xb.ptr, rs, tb.ptr, -100, rows, P, acc[0].ptr, acc[1].ptr, gb.ptr, gs_, sp()))
    else:
        _lib.check(L().pk2_softmax_ce_fwd_bwd(xb.ptr, rs, tb.ptr, -100, rows, P, acc[0].ptr, acc[1].ptr, gb.ptr if gb else None, gs_,
                                              lb.ptr if lb else None, sp()))
    torch.cuda.synchronize()
    for b in (acc[0], acc[1], gb, lb):
        assert b is None or b.bands_intact(), "a write outside an output of the CE call"
    grad = None
    if gb:
        g = gb.host()
        assert (g[:, P:] == S).all(), "a write into the gap behind a gradient row"
        grad = g[:, :P]
    return dict(loss=float(acc[0].host()[0]), count=int(acc[1].host()[0]), grad=grad, lp=lb.host() if lb else None, acc=acc)


def check_ce(x, t, res, mean, tag=""):
    """Holds one result of run_ce to the oracle.  Returns the measured (gradient error / gs, log-prob error, log-prob bound)."""
    loss_sum, count, grad64, lp64 = ce_ref.cross_entropy(x, t, -100, "mean" if mean else "sum")
    gs = 1.0 / max(1, count) if mean else 1.0
    assert res["count"] == count, (tag, res["count"], count)
    if np.isnan(loss_sum):
        assert np.isnan(res["loss"]), (tag, res["loss"])
    else:
        assert np.isfinite(res["loss"]), (tag, res["loss"])
        assert abs(res["loss"] - loss_sum) <= E.CE_LOSS_REL * abs(loss_sum), (tag, res["loss"], loss_sum)
    gerr = lerr = bound = 0.0
    if res["grad"] is not None:
        assert np.isfinite(res["grad"]).all(), (tag, "gradient not finite (unwritten, or a read outside the row)")
        err = np.abs(res["grad"].astype(np.float64) - grad64)
        gerr = float(err.max()) / gs
        r = int(err.max(axis=1).argmax())
        assert gerr <= E.CE_GRAD_BOUND, (tag, "row %d" % r, gerr)
        valid, _ = ce_ref.valid_rows(t, x.shape[1])
        assert not res["grad"][~valid].any(), (tag, "gradient of an ignored row is not zero")
    if res["lp"] is not None:
        bound, e_torch, floor = E.logprob_bound(x, lp64)
        lerr = E.logprob_error(res["lp"], lp64)
        assert lerr <= bound, (tag, "log-probs", lerr, bound, e_torch)
    if x.shape[0] == 1 and count == 1:                 # one row: the loss is that row's loss, held to the log-prob bound
        bound, e_torch, floor = E.logprob_bound(x, lp64)
        lerr = max(lerr, abs(res["loss"] - loss_sum))
        assert abs(res["loss"] - loss_sum) <= bound, (tag, "row loss", res["loss"], loss_sum, bound)
    return gerr, lerr, bound


def edge_targets(P, rows=3):
    """class 0, class P-1, and a class in the last partial 256-chunk of the row."""
    last = ((P - 1) // 256) * 256
    return np.asarray([0, P - 1, last + (P - 1 - last) // 2][:rows] * (rows // 3 + 1), np.int64)[:rows]


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 517, 8191, 8192, 8193, 9000, 20011])
def test_ce_class_counts_around_every_chunk_and_variant_edge(P, mean):
    """8192 is the last width of the register variant, 8193 the first of the streaming one; targets on class 0, class P-1
    and in the last partial 256-chunk."""
    x = E.ce_logits("spread", 3, P)
    t = edge_targets(P)
    check_ce(x, t, run_ce(x, t, mean), mean, "P=%d" % P)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("P", [70, 9000])
@pytest.mark.parametrize("regime", E.CE_REGIMES)
def test_ce_regimes_gradient_loss_and_log_probs(regime, P, rows):
    """Both variants (P = 70 in registers, P = 9000 streaming; with logprob_out the streaming one at both widths), the sum and
    the mean call.  Per-row loss: rows = 1, and logprob_out[row, target].  Bounds: gradient 2e-6 * gs; log-probs and row
    loss 4 e_torch + 8 * 2^-23 * max(1, max |lp64|); the float32 CPU model of (x - m) - log s stays under half of that
    (tests/test_oracle_ce_optim.py), x - (m + log s) reaches 4 to 6 times the bound in `offset`.
    Three figures per bound (CPU float32 model | measured on the MI355X | margin to the bound), worst over P and rows:
      log-probs / row loss   spread 1.4e-6 | 1.4e-6 | 16x    peaked 1.4e-5 | 1.4e-5 | 21x
                             offset 8.1e-7 | 8.1e-7 | 36x    masked 1.9e-6 | 2.1e-6 | 16x
      gradient (2e-6)        1e-6 in the model (offset, exp(lp) - onehot) | 1.1e-7 measured | 17x
    The kernel lands on torch's own float32 error (e_torch) to two digits.  Before the maximum was subtracted first the
    same cases measured, in `offset`: row loss 4.6e-5 against a bound of 1.8e-5 (P = 70, register variant), gradient 1.1e-5 to
    2.8e-5 against 2e-6 (streaming variant); and in `peaked` at P = 9000 a gradient of 2.5e-6."""
    x = E.ce_logits(regime, rows, P)
    t = E.ce_targets(x)
    worst = [0.0, 0.0, 0.0]
    for mean, lp in ((False, False), (True, False), (False, True)):
        g, le, b = check_ce(x, t, run_ce(x, t, mean, want_lp=lp), mean, "%s P=%d rows=%d mean=%d lp=%d" % (regime, P, rows, mean, lp))
        worst = [max(worst[0], g), max(worst[1], le), max(worst[2], b)]
    print("CE %-6s P=%d rows=%d: gradient error %.2e (bound %.0e), log-prob / row-loss error %.2e (bound %.2e)"
          % (regime, P, rows, worst[0], E.CE_GRAD_BOUND, worst[1], worst[2]))


@pytest.mark.parametrize("mean", [False, True])
def test_ce_rows_walked_by_a_workgroup(mean):
    """rows = 2 * 2048 + 5 at the grid cap of 2048 workgroups: a workgroup takes two or three rows.  Every seventh row ignored;
    every row's gradient, the count and the loss are checked, then once more with one target out of range (NaN loss, that
    row's gradient zero, one less counted)."""
    rows, P = 4101, 70
    x = E.ce_logits("spread", rows, P)
    t = E.ce_targets(x)
    t[::7] = -100
    check_ce(x, t, run_ce(x, t, mean), mean, "walk")
    t[2049] = P
    res = run_ce(x, t, mean)
    check_ce(x, t, res, mean, "walk, one target out of range")
    assert np.isnan(res["loss"]) and not res["grad"][2049].any()


@pytest.mark.parametrize("P", [70, 9000])
def test_ce_row_strides(P):
    """row_stride = P + 3 with NaN in the gaps, grad_row_stride = P + 5 with SENTINEL in the gaps (run_ce checks them)."""
    x = E.ce_logits("spread", 5, P)
    t = E.ce_targets(x)
    t[3] = -100
    for mean, lp in ((False, False), (True, False), (False, True)):
        check_ce(x, t, run_ce(x, t, mean, row_stride=P + 3, grad_stride=P + 5, want_lp=lp), mean, "strides P=%d" % P)


@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("P", [70, 9000])
def test_ce_logprob_out_with_and_without_gradient(P, with_grad):
    """logprob_out holds log_softmax of EVERY row, ignored and out-of-range ones included (their gradient rows are zero)."""
    x = E.ce_logits("spread", 6, P)
    t = E.ce_targets(x)
    t[1] = t[4] = -100
    res = run_ce(x, t, False, want_grad=with_grad, want_lp=True)
    check_ce(x, t, res, False, "lp")
    t[5] = -3
    res = run_ce(x, t, False, want_grad=with_grad, want_lp=True)
    check_ce(x, t, res, False, "lp, out of range")
    # neither gradient nor log-probs: loss and count alone
    t[5] = 0
    check_ce(x, t, run_ce(x, t, False, want_grad=False), False, "loss only")


@pytest.mark.parametrize("P", [70, 9000])
def test_ce_all_targets_ignored_and_repeated_call(P):
    x = E.ce_logits("spread", 3, P)
    for mean in (False, True):
        res = run_ce(x, [-100] * 3, mean)
        assert res["loss"] == 0.0 and res["count"] == 0 and not res["grad"].any()
    # the accumulators are zeroed inside: a second call on the same pair gives the same loss (one row: the same bits)
    for rows in (1, 300):
        x = E.ce_logits("spread", rows, P if rows == 1 else 70)
        t = E.ce_targets(x)
        for mean in (False, True):
            a = run_ce(x, t, mean)
            b = run_ce(x, t, mean, acc=a["acc"])
            assert b["count"] == a["count"] == rows
            assert b["loss"] == a["loss"] if rows == 1 else abs(b["loss"] - a["loss"]) <= 1e-6 * abs(a["loss"])
            assert np.array_equal(a["grad"], b["grad"])


@pytest.mark.parametrize("red", ["mean", "sum"])
def test_cross_entropy_loss_module_on_the_time_major_view_streaming(red):
    """ops.CrossEntropyLoss at P = 9000 on x.transpose(0, 1) of a contiguous [T, B, P] (what LSTMAM returns): rows are taken
    in memory order, targets follow, the gradient comes back in the view's layout."""
    T, B, P = 5, 3, 9000
    x = E.ce_logits("spread", T * B, P).reshape(T, B, P)
    t = E.ce_targets(x.reshape(T * B, P)).reshape(T, B)
    t[4, 1] = t[0, 2] = -100
    xd = torch.from_numpy(x).cuda().requires_grad_()
    loss = ops.CrossEntropyLoss(ignore_index=-100, reduction=red)(xd.transpose(0, 1), torch.from_numpy(t).cuda().transpose(0, 1))
    loss.backward()
    loss_sum, count, grad64, _ = ce_ref.cross_entropy(x.reshape(T * B, P), t.reshape(-1), -100, red)
    want = ce_ref.reduce_loss(loss_sum, count, red)
    assert abs(loss.item() - want) <= E.CE_LOSS_REL * abs(want)
    gs = 1.0 / count if red == "mean" else 1.0
    assert np.abs(xd.grad.cpu().numpy().astype(np.float64) - grad64.reshape(T, B, P)).max() <= E.CE_GRAD_BOUND * gs


SCALE_SIZES = (1, 3, 4, 5, 1027, 4 * 4096 * 256 + 4099)        # the last: the float4 grid-stride loop goes round


def _scale_expect(x, num, den):
    """The float32 statement x * (num / den)."""
    return x * (np.float32(num) / np.float32(den))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SCALE_SIZES)
def test_scale_kernels_are_the_float32_statement(n, off):
    """pk2_scale_inplace_ratio, pk2_scale_by_scalars and pk2_scale_by_count against x * (num / den) in float32, bit for bit
    (hipcc divides correctly rounded by default and the kernels multiply once: measured equal on the MI355X, no 2-ulp
    allowance needed).  off = 1: a base one float off 16-byte alignment takes the scalar path and must stay inside."""
    rng = np.random.default_rng(n + off)
    x = rng.standard_normal(n).astype(np.float32)
    scal = lambda v, dt=np.float32: Buf(np.asarray([v], dt), dt(-7))       # noqa: E731
    # in place: num / den, den = NULL, factor exactly 1 (nothing touched)
    for num, den in ((0.37, 1.7), (-2.5, None), (3.0, 3.0)):
        d = Buf(x, S, off)
        nb, db = scal(num), scal(den) if den is not None else None
        _lib.check(L().pk2_scale_inplace_ratio(d.ptr, n, nb.ptr, db.ptr if db else None, sp()))
        torch.cuda.synchronize()
        assert np.array_equal(d.host(), _scale_expect(x, num, 1.0 if den is None else den)) and d.bands_intact(), (num, den)
    # out of place and out == in: mul / max(1, count); either scalar NULL; count = 0
    for mul, cnt, inplace in ((0.37, 20, False), (None, 7, False), (1.5, None, False), (-0.25, 0, False), (0.37, 20, True)):
        src = Buf(x, S if inplace else np.float32(np.nan), off)
        dst = src if inplace else out_f32(n, off)
        mb, cb = scal(mul) if mul is not None else None, scal(cnt, np.int32) if cnt is not None else None
        _lib.check(L().pk2_scale_by_scalars(src.ptr, dst.ptr, n, mb.ptr if mb else None, cb.ptr if cb else None, sp()))
        torch.cuda.synchronize()
        want = _scale_expect(x, 1.0 if mul is None else mul, max(1, cnt or 1))
        assert np.array_equal(dst.host(), want) and dst.bands_intact(), (mul, cnt, inplace)
    for numer, cnt in ((1.0, 20), (0.5, 0), (-3.0, 1)):
        d = Buf(x, S, off)
        cb = scal(cnt, np.int32)
        _lib.check(L().pk2_scale_by_count(d.ptr, n, numer, cb.ptr, sp()))
        torch.cuda.synchronize()
        assert np.array_equal(d.host(), _scale_expect(x, numer, max(1, cnt))) and d.bands_intact(), (numer, cnt)


# ================================================================================================================ optimisers
class _Flat:
    """The model interface of optim._FlatOptimizer over two given flat tensors."""

    def __init__(self, p, g):
        self.p, self.g = p, g

    def flat_parameters(self):
        return self.p, self.g

    def parameters(self):
        return [self.p]


def _check_traj(tag, k, got, t64, worst):
    """got: {tensor name: float32 array} after step k, against the float64 trajectory, at tests/edge_cases.opt_bound."""
    for key, val in got.items():
        assert np.isfinite(val).all(), (tag, k, key)
        err = float(np.abs(val.astype(np.float64) - t64[k][key]).max())
        bound = E.opt_bound(key, t64, k)
        worst[key] = max(worst.get(key, 0.0), err / bound)
        assert err <= bound, (tag, "step %d" % (k + 1), key, err, bound)


@pytest.mark.parametrize("n", E.OPT_SIZES)
def test_grad_norm_sizes_tail_and_grid_stride(n):
    """pk2_grad_norm: n % 4 tails, n / 4 beyond 1024 * 256 float4 (the grid-stride loop goes round).  Relative error <= 1e-6: a
    sum of non-negative float32 pair-squares carries at most 2 ulp, accumulated in double; the root halves it; one rounding to
    float: about 2e-7, times 5.  A float32 rounding of the exact norm alone is up to 6e-8; measured on the MI355X: at most
    4.1e-8 (n = 2 * 4096 * 256 + 3), 24x inside."""
    p0, grads = E.opt_problem(n)
    for g in (grads[3], grads[0]):
        gb, nb, ws = in_f32(g), out_f32(1), Buf(np.full(2048, np.nan, np.float32), S)
        assert L().pk2_grad_norm_workspace_bytes(n) <= 2048 * 4
        _lib.check(L().pk2_grad_norm(gb.ptr, n, nb.ptr, ws.ptr, 2048 * 4, sp()))
        torch.cuda.synchronize()
        want = optim_ref.grad_norm(g)
        got = float(nb.host()[0])
        assert nb.bands_intact() and ws.bands_intact()
        print("norm n=%d: relative error %.1e" % (n, abs(got - want) / want if want > 0 else 0.0))
        assert abs(got - want) <= E.NORM_REL * want if want > 0 else got == 0.0, (n, got, want)


def _abi_adam(n, amsgrad, wd, gs, clip):
    p0, grads = E.opt_problem(n)
    t64 = E.run_adam(p0, grads, amsgrad, wd, gs, clip, np.float64)
    z = np.zeros(n, np.float32)
    p, m, v, vm = Buf(p0, S), Buf(z, S), Buf(z, S), Buf(z, S) if amsgrad else None
    nb, ws = out_f32(1), Buf(np.zeros(2048, np.float32), S)
    worst = {}
    for k in range(E.OPT_STEPS):
        g = in_f32(grads[k])
        measured = clip != "none"
        if measured:
            _lib.check(L().pk2_grad_norm(g.ptr, n, nb.ptr, ws.ptr, 2048 * 4, sp()))
        # (the clip acts on the scaled gradient: max_norm / grad_scale against the norm of the unscaled one, as optim.py passes it)
        _lib.check(L().pk2_adam_step(p.ptr, g.ptr, m.ptr, v.ptr, vm.ptr if vm else None, n, E.OPT_LRS[k], E.OPT_BETAS[0], E.OPT_BETAS[1], 1e-8, wd, k + 1,
                                     E.OPT_MAX_NORM[clip] / gs if measured else 0.0, nb.ptr if measured else None, gs, sp()))
        torch.cuda.synchronize()
        got = dict(p=p.host(), exp_avg=m.host(), exp_avg_sq=v.host())
        if vm:
            got["max_exp_avg_sq"] = vm.host()
        _check_traj("adam n=%d" % n, k, got, t64, worst)
        assert all(b.bands_intact() for b in (p, m, v, vm, nb) if b is not None)
    if wd == 0:
        assert p.host()[n // 2] == p0[n // 2]              # an exactly-zero gradient: 0 / (0 + eps) moves nothing
    return worst


def _abi_sgd(n, momentum, wd, gs, clip):
    p0, grads = E.opt_problem(n)
    t64 = E.run_sgd(p0, grads, momentum, wd, gs, clip, np.float64)
    # the momentum buffer starts as NaN: the first step must not read it (buf = d)
    p, buf = Buf(p0, S), Buf(np.full(n, np.nan, np.float32), S) if momentum else None
    nb, ws = out_f32(1), Buf(np.zeros(2048, np.float32), S)
    worst = {}
    for k in range(E.OPT_STEPS):
        g = in_f32(grads[k])
        measured = clip != "none"
        if measured:
            _lib.check(L().pk2_grad_norm(g.ptr, n, nb.ptr, ws.ptr, 2048 * 4, sp()))
        _lib.check(L().pk2_sgd_step(p.ptr, g.ptr, buf.ptr if buf else None, n, E.OPT_LRS[k], momentum, wd, 1 if k == 0 else 0,
                                    E.OPT_MAX_NORM[clip] / gs if measured else 0.0, nb.ptr if measured else None, gs, sp()))
        torch.cuda.synchronize()
        got = dict(p=p.host())
        if buf:
            got["buf"] = buf.host()
        _check_traj("sgd n=%d" % n, k, got, t64, worst)
        assert all(b.bands_intact() for b in (p, buf, nb) if b is not None)
    if wd == 0:
        assert p.host()[n // 2] == p0[n // 2]
    return worst


@pytest.mark.parametrize("n", [n for n in E.OPT_SIZES if n != 1000])
def test_adam_and_sgd_sizes_through_the_c_abi(n):
    """Ten steps at every size, one variant each (amsgrad / momentum on for odd n): n = 2 * 4096 * 256 + 3 makes the grid-stride
    loops of adam_kernel, sgd_kernel and sumsq_partial go round and leaves an n % 4 tail.  Parameters AND moments against
    optim_ref in float64 at a k ulp(max |p|) + b k lr, a = 2.2, b = 1.9e-6, and 11.2 k ulp(max |moment|): four times what the
    float32 mode of optim_ref loses (0.50 k ulp on p, 2.8 k ulp on exp_avg_sq; tests/test_oracle_ce_optim.py).
    Three figures per bound, as fractions of it (CPU float32 model | measured on the MI355X | margin): parameters
    0.23 | 0.23 | 4.4x (Adam and SGD alike); moments 0.25 | 0.20 | 5x.  The kernels lose what the model loses."""
    flag, wd, gs, clip = E.opt_size_case(n)
    wa = _abi_adam(n, flag, wd, gs, clip)
    ws = _abi_sgd(n, 0.9 if flag else 0.0, wd, gs, clip)
    print("n=%d error / bound: adam %s  sgd %s" % (n, {k: round(v, 3) for k, v in wa.items()}, {k: round(v, 3) for k, v in ws.items()}))


@pytest.mark.parametrize("flag,wd,gs,clip", itertools.product((True, False), (0.0, 0.01), (1.0, 0.125), ("none", "binding", "loose")))
def test_adam_and_sgd_variants_at_n_1000(flag, wd, gs, clip):
    """The cross product amsgrad (momentum 0.9 / 0 for SGD) x weight_decay x grad_scale x clip {not measured, binding, measured
    and not binding} through the C ABI, and the same through optim.Adam / optim.SGD / clip_grad_norm_ with opt.grad_scale and
    lr rewritten between steps: the wrapper must hand the kernel max_norm / grad_scale and return the norm of the SCALED
    gradient."""
    n = 1000
    wa = _abi_adam(n, flag, wd, gs, clip)
    ws = _abi_sgd(n, 0.9 if flag else 0.0, wd, gs, clip)
    print("error / bound: adam %s  sgd %s" % ({k: round(v, 3) for k, v in wa.items()}, {k: round(v, 3) for k, v in ws.items()}))
    p0, grads = E.opt_problem(n)
    for name in ("adam", "sgd"):
        pb, gb = Buf(p0, S), Buf(np.zeros(n, np.float32), np.float32(np.nan))
        model = _Flat(pb.t, gb.t)
        if name == "adam":
            opt = optim.Adam(model, lr=1.0, betas=E.OPT_BETAS, weight_decay=wd, amsgrad=flag)
            t64 = E.run_adam(p0, grads, flag, wd, gs, clip, np.float64)
        else:
            opt = optim.SGD(model, lr=1.0, momentum=0.9 if flag else 0.0, weight_decay=wd)
            t64 = E.run_sgd(p0, grads, 0.9 if flag else 0.0, wd, gs, clip, np.float64)
        opt.grad_scale = gs
        worst = {}
        for k in range(E.OPT_STEPS):
            opt.zero_grad()
            gb.t.copy_(torch.from_numpy(grads[k]))
            opt.param_groups[0]["lr"] = E.OPT_LRS[k]
            if clip != "none":
                norm = optim.clip_grad_norm_(opt, E.OPT_MAX_NORM[clip]).item()
                assert abs(norm - t64[k]["norm"]) <= E.NORM_REL * t64[k]["norm"], (name, k, norm, t64[k]["norm"])
            opt.step()
            torch.cuda.synchronize()
            got = dict(p=pb.host())
            if name == "adam":
                got.update(exp_avg=opt.state["exp_avg"].cpu().numpy(), exp_avg_sq=opt.state["exp_avg_sq"].cpu().numpy())
                if flag:
                    got["max_exp_avg_sq"] = opt.state["max_exp_avg_sq"].cpu().numpy()
                else:
                    assert opt.state["max_exp_avg_sq"] is None
            elif flag:
                got["buf"] = opt.buf.cpu().numpy()
            else:
                assert opt.buf is None
            _check_traj(name + " wrapper", k, got, t64, worst)
        assert pb.bands_intact()


# ================================================================================================================== front end
@functools.lru_cache(maxsize=None)
def _mel():
    return fbank.mel_filterbank()


@functools.lru_cache(maxsize=None)
def _utt(kind, n, seed=0):
    """(waveform, float64 log-mel oracle with the library's one zero-padded frame for utterances under 242 samples, the
    CPU model of the kernel's arithmetic on the same utterance)."""
    w = E.signal(kind, n, seed)
    return w, F.logfbank64(w, _mel(), pad_short=True), F.logfbank_model(w, _mel(), pad_short=True)


def run_fbank(fb, utts, cmn):
    """pk2_fbank_compute on the utterances [(kind, samples)] back to back.  Returns (feats [rows, 80], row offsets)."""
    wavs = [_utt(k, n, i)[0] for i, (k, n) in enumerate(utts)]
    lens = [w.shape[0] for w in wavs]
    frames = [fbank.num_frames(v) for v in lens]
    wav_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    wb, ro, out = in_f32(np.concatenate(wavs)), Buf(row_off, np.int64(-1)), out_f32((int(row_off[-1]), 80))
    _lib.check(L().pk2_fbank_compute(fb._h, wb.ptr, _lib.ptr(wav_off), len(utts), out.ptr, ro.ptr, 1 if cmn else 0, sp()))
    torch.cuda.synchronize()
    assert out.bands_intact(), "a write outside the feature matrix"
    return out.host(), row_off


def test_frame_counts_at_the_edges():
    """From 242 samples up the reference's count; 2...241 samples: the library's present answer, ONE zero-padded frame, where
    the reference's _enframe produces none (pinned, not endorsed: DESIGN.md)."""
    for n in E.FBANK_SAMPLES + tuple(range(242, 1500, 7)):
        if n >= 242:
            assert fbank.num_frames(n) == F.enframe_pad(np.zeros(n - 1)).shape[0], n
    assert [fbank.num_frames(n) for n in (401, 402, 561, 562, 16001)] == [1, 2, 2, 3, 99]
    assert all(fbank.num_frames(n) == 1 for n in range(2, 242)) and F.enframe_pad(np.zeros(240)).shape[0] == 0
    assert fbank.num_frames(1) == 0 and fbank.num_frames(0) == 0


@pytest.mark.parametrize("cmn", [False, True])
@pytest.mark.parametrize("num_utts", [1, 32, 33, 65])
def test_fbank_ragged_batches_across_the_per_32_launches(num_utts, cmn):
    """1, 32, 33 and 65 utterances in one call (one, one, two and three launches with a running row offset), lengths cycling
    through the frame-count edges and signals through the five regimes (65 utterances: all 45 pairs).  Every utterance's rows
    must land at its row offset.  All-zero signals give exactly 0, one-frame utterances exactly 0 after CMN.
    Two bounds against logfbank64 (logfbank, the reference's complex64 path, is 1.2e-6 from it):
      * 2e-4, the project's existing fbank bound;
      * tests/edge_cases.fbank_tight_bound, 4 x the CPU model of the kernel's arithmetic + 4 * 2^-23 * max |log-mel|
        (about 1.5e-5): it holds the float32 pre-emphasis to its two roundings.
    CPU model per regime: noise 1.2e-6, quiet 3.9e-7, square 1.1e-6, tone 1.0e-6, zeros 0; tight bound 1.7e-5 (quiet 5e-6).
    Measured on the MI355X while the pre-emphasis was still ONE fused multiply-add: noise 2.2e-5, tone 6.8e-5 (both over
    the tight bound; the CPU model of that fma gives the same 6.8e-5), square 3.9e-6, quiet 1.1e-6, zeros 0.  With the
    two roundings restored (v_mul_f32, v_sub_f32 in the disassembly) the test prints model, measured value and their
    ratio to the tight bound per regime; the device figures of that build are not recorded here yet."""
    fb = fbank.FbankExtractor()
    utts = [(E.SIGNALS[(i + num_utts) % 5], E.FBANK_SAMPLES[(i + 2 * num_utts) % 9]) for i in range(num_utts)]
    feats, row_off = run_fbank(fb, utts, cmn)
    assert np.isfinite(feats).all(), "unwritten feature rows"
    worst = {}
    for i, (kind, n) in enumerate(utts):
        _, want, model = _utt(kind, n, i)
        got = feats[row_off[i]:row_off[i + 1]]
        assert got.shape == want.shape, (i, kind, n)
        tight, e_model = E.fbank_tight_bound(model, want)
        if cmn:
            want = F.cmn(want)
        err = float(np.abs(got - want).max())
        w = worst.setdefault(kind, [0.0, 0.0, 0.0])
        worst[kind] = [max(w[0], e_model), max(w[1], err), max(w[2], err / tight)]
        assert err <= E.FBANK_BOUND, (i, kind, n, err)
        assert err <= tight, (i, kind, n, err, tight, e_model)
        if kind == "zeros" or (cmn and got.shape[0] == 1):
            assert not got.any(), (i, kind, n)
    print("fbank%s, %d utterances, per regime (model, measured, measured / tight bound): %s"
          % (" + CMN" if cmn else "", num_utts, {k: "%.1e %.1e %.2f" % tuple(v) for k, v in worst.items()}))
    if num_utts == 33:          # the wrapper: the same rows, its frame list and row offsets
        wav = torch.from_numpy(np.concatenate([_utt(k, n, i)[0] for i, (k, n) in enumerate(utts)])).cuda()
        f2, frames, ro = fb(wav, [n for _, n in utts], apply_cmn=cmn)
        assert np.array_equal(ro.cpu().numpy(), row_off) and list(frames) == list(np.diff(row_off))
        assert np.array_equal(f2.cpu().numpy(), feats)


def test_cmn_partition_and_unroll_tails():
    """T in {1, 11, 12, 13, 47, 48, 49}: fewer frames than the 12 partitions, exactly 12, the 4x unrolled loop's first full
    round (48) and the frames on either side.  Against cmn(logfbank64) at the fbank bound, and against the mean of the
    kernel's own uncentred features in float64 at 2^-23 * max |x| (the mean rounded to float32, one subtraction: half an
    ulp of the mean plus half an ulp of the difference, log-mels being non-negative).  Three figures for that bound, as
    fractions of it: the float32 CPU statement x - float32(mean) reaches at most 1 by construction (half an ulp of the
    mean, half an ulp of the difference, in ulps of max |x|); the test prints model and measured value side by side."""
    fb = fbank.FbankExtractor()
    Ts = (1, 11, 12, 13, 47, 48, 49)
    utts = [("noise", 401 + 160 * (T - 1)) for T in Ts]
    raw, row_off = run_fbank(fb, utts, False)
    got, _ = run_fbank(fb, utts, True)
    assert list(np.diff(row_off)) == list(Ts)
    ratios = [0.0, 0.0]
    for i, T in enumerate(Ts):
        a, b = row_off[i], row_off[i + 1]
        want = F.cmn(_utt(*utts[i], i)[1])
        assert np.abs(got[a:b] - want).max() <= E.FBANK_BOUND, T
        own = raw[a:b].astype(np.float64)
        centred = own - own.mean(0, keepdims=True)
        model = raw[a:b] - own.mean(0, keepdims=True).astype(np.float32)          # float32 - float32, rounded once
        bound = E.ULP * np.abs(own).max()
        ratios = [max(ratios[0], np.abs(model - centred).max() / bound), max(ratios[1], np.abs(got[a:b] - centred).max() / bound)]
        assert np.abs(got[a:b] - centred).max() <= bound, T
        if T == 1:
            assert not got[a:b].any()
    print("CMN error / bound: float32 model %.2f, measured %.2f" % tuple(ratios))


def _frames_for(N, max_t):
    fr = [1 + (5 * i + 3) % max_t for i in range(N)]
    fr[N // 2] = max_t
    fr[0] = 1
    if N == 1:
        fr[0] = max_t
    return fr


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("N,max_t", [(1, 1), (1, 7), (5, 13), (33, 23)])
def test_pad_roll_subsample_edges_bit_equal(N, max_t, time_major):
    """subsample 1...4 with max_t no multiple of it, shift 0, -1, -2 and -(max_t + 1) (the header allows shift <= 0), frame
    counts including 1, both layouts: bit-equal to frontend_ref.pad_roll_subsample."""
    frames = _frames_for(N, max_t)
    _pad_roll_case(frames, [(s, sh) for s in (1, 2, 3, 4) for sh in (0, -1, -2, -(max_t + 1))], time_major)


@pytest.mark.parametrize("time_major", [False, True])
def test_pad_roll_subsample_beyond_the_grid_cap(time_major):
    """N = 33, max_t = 1600: 33 * 1600 * 20 float4 exceed 4096 workgroups of 256 -- the grid-stride loop goes round."""
    frames = [1 + (131 * i) % 1600 for i in range(33)]
    frames[7] = 1600
    _pad_roll_case(frames, [(1, -2)], time_major)


def _pad_roll_case(frames, variants, time_major):
    N, max_t = len(frames), max(frames)
    rng = np.random.default_rng(N * 100 + max_t)
    feats = rng.standard_normal((sum(frames), 80)).astype(np.float32)
    row_off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    fbuf, ro = in_f32(feats), Buf(row_off, np.int64(-1))
    flist = np.split(feats, row_off[1:-1])
    for sub, shift in variants:
        want = F.pad_roll_subsample(flist, shift=shift, subsample=sub)
        out_t = (max_t - 1) // sub + 1
        assert want.shape == (N, out_t, 80)
        out = out_f32((out_t, N, 80) if time_major else (N, out_t, 80))
        _lib.check(L().pk2_pad_roll_subsample(fbuf.ptr, ro.ptr, N, max_t, shift, sub, out.ptr, out_t, 1 if time_major else 0, sp()))
        torch.cuda.synchronize()
        got = out.host()
        assert out.bands_intact()
        assert np.array_equal(got.transpose(1, 0, 2) if time_major else got, want), (sub, shift)
    # the wrapper computes max_t and out_t itself
    x = fbank.FbankExtractor.pad_roll_subsample(fbuf.t.view(-1, 80), ro.t, frames, shift=variants[-1][1], subsample=variants[-1][0],
                                                time_major=time_major)
    assert np.array_equal(x.cpu().numpy(), got)


@pytest.mark.parametrize("rows", [1, 7, 60000])
@pytest.mark.parametrize("dim", [1, 40, 80, 83])
def test_mvn_apply_dims_and_grid_cap(dim, rows):
    """(x - mean) / std elementwise against float64 on the float32 inputs at 4 * 2^-24 * |y|: two correctly rounded operations
    (hipcc's default float division is correctly rounded; the library is not built with a fast one) with margin.  60000 rows
    pass the cap of 4096 workgroups from dim = 40 up.  In units of 2^-24 |y| (bound 4): the float32 CPU statement
    (x - mean) / std on the same data reaches 1.98; the device performs the same two correctly rounded operations and
    passed this bound; the test prints model and measured value per case."""
    rng = np.random.default_rng(dim * 7 + rows)
    x = (5 * rng.standard_normal((rows, dim)) + 3).astype(np.float32)
    mean = (3 * rng.standard_normal(dim)).astype(np.float32)
    std = rng.uniform(0.01, 3.0, dim).astype(np.float32)
    want = F.mvn_apply(x.astype(np.float64), mean.astype(np.float64), std.astype(np.float64))
    xb, mb, sb, out = in_f32(x), in_f32(mean), in_f32(std), out_f32((rows, dim))
    _lib.check(L().pk2_mvn_apply(xb.ptr, mb.ptr, sb.ptr, rows, dim, out.ptr, sp()))
    torch.cuda.synchronize()
    got = out.host()
    assert out.bands_intact() and np.isfinite(got).all()
    model = (x - mean) / std                                         # the float32 statement on the CPU
    rel = lambda v: float((np.abs(v - want) / np.maximum(np.abs(want), 1e-300)).max() / 2.0 ** -24)       # noqa: E731
    print("mvn dim=%d rows=%d, error in units of 2^-24 |y| (bound 4): float32 model %.2f, measured %.2f" % (dim, rows, rel(model), rel(got)))
    assert (np.abs(got - want) <= 4 * 2.0 ** -24 * np.abs(want)).all(), rel(got)
    if rows == 7:               # the wrapper: [.., dim] tensors of any leading shape
        mvn = fbank.GlobalMeanVarianceNormalization(mean, std)
        assert np.array_equal(mvn(xb.t.view(rows, dim)).cpu().numpy(), got)
