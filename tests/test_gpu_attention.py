"""The fused attention kernels (csrc/attention.hip), the row kernels of TransformerAM (csrc/transformer_ops.hip) and the
counter-based dropout mask (csrc/dropout.hip) through the C ABI, against the numpy oracles oracle/attention_ref.py and
oracle/dropout_ref.py.

Every tensor X of a case is held to the bound of tests/bound_check.py (the LSTM tests' bound, unchanged):

    max |X - X_float64-oracle|  <=  4 * max(e32(X), 2^-23 * max |X_float64-oracle|)

with e32 the error of the float32 oracle on the same data; where the float64 lse is -inf the result must be -inf.  Every
attention case runs pk2_attention_fwd, then pk2_attention_bwd on the kernel's own ctx / lse.  Outputs are pre-filled with
NaN inside a larger allocation whose bands in front and behind hold a bit pattern that must survive; inputs sit between
bands of NaN, so that a read outside them poisons a result.  The dropout mask of the oracle is dropout_ref's, never the
device's.  One line per (case, tensor) is printed: attention_ratio | case | tensor | ratio.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_check as A
import bound_check
from oracle import attention_ref, dropout_ref
from pykaldi2_amd import _lib

pytestmark = pytest.mark.gpu

# tensor -> factor, for a tensor that needs more than bound_check.FACTOR: only with the arithmetic step that costs it named here.
FACTORS = {}
CANARY = 0x5A17C0DE            # bit pattern of the bands around an output (a finite float)


class Guarded:
    """A device array inside a larger allocation with a band in front of it and behind it.  Inputs (data given): the bands
    are NaN (float32).  A key-padding array (uint8) cannot hold NaN: the band in front of it is 1 (padded), the band behind it
    0 (a valid key), so that a read in front of it masks keys that are valid and a read behind it lets padded keys in -- either
    changes a number wherever the neighbouring utterance differs from the band, and every padded case here has both kinds of
    utterance.  Outputs (n given): the array is NaN, the bands hold CANARY.  inout: data given, CANARY bands (operators that
    work in place)."""

    def __init__(self, data=None, n=None, band=256, inout=False):
        self.host = None if data is None else np.ascontiguousarray(data)
        self.n = int(n if data is None else self.host.size)
        self.band = band = (int(band) + 255) // 256 * 256
        self.checked = data is None or inout
        if self.host is not None and self.host.dtype == np.uint8:
            self.buf = torch.zeros(2 * band + self.n, dtype=torch.uint8, device="cuda")
            self.buf[:band] = 1
        else:
            assert self.host is None or self.host.dtype == np.float32
            bits = torch.full((2 * band + self.n,), CANARY, dtype=torch.int32, device="cuda")
            self.buf = bits.view(torch.float32)
            if not self.checked:
                self.buf.fill_(float("nan"))
        self.t = self.buf[band:band + self.n]
        if self.host is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(torch.from_numpy(self.host.ravel()))
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:self.band] == CANARY).all()) and bool((bits[self.band + self.n:] == CANARY).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.uint8), self.host.ravel().view(np.uint8))


def _opt(g):
    return g.ptr if g is not None else None


def _report(label, failures, ratios, problems):
    for name, r in ratios.items():
        print("attention_ratio | %s | %s | %.3f" % (label, name, r))
    problems += ["%s: %s" % (label, msg) for _, msg in failures]


def run_attention(case, label):
    """Forward, then backward on the kernel's own ctx / lse; memory hygiene, the bound, exact zeros at padded keys.
    Returns the device results."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    T, B, H = case["T"], case["B"], case["H"]
    Cc = H * 64
    qkv, dctx = Guarded(case["qkv"], band=2 * 3 * Cc), Guarded(case["dctx"], band=2 * Cc)
    src = Guarded(case["src_mask"], band=2 * T) if case["src_mask"] is not None else None
    pad = Guarded(case["key_padding"], band=2 * T) if case["key_padding"] is not None else None
    ctx, dq = Guarded(n=T * B * Cc, band=2 * Cc), Guarded(n=T * B * 3 * Cc, band=2 * 3 * Cc)
    lse, dsum = Guarded(n=B * H * T, band=2 * T), Guarded(n=B * H * T, band=2 * T)
    seed = C.c_uint64(case["seed"])
    _lib.check(L.pk2_attention_fwd(qkv.ptr, T, B, H, 64, case["scale"], _opt(src), _opt(pad), case["p"], seed, ctx.ptr, lse.ptr, sp))
    torch.cuda.synchronize()
    _lib.check(L.pk2_attention_bwd(qkv.ptr, ctx.ptr, dctx.ptr, lse.ptr, T, B, H, 64, case["scale"], _opt(src), _opt(pad), case["p"],
                                   seed, dq.ptr, dsum.ptr, sp))
    torch.cuda.synchronize()
    problems = []
    for name, g in (("ctx", ctx), ("lse", lse), ("dqkv", dq), ("dsum", dsum)):
        if not g.intact():
            problems.append("%s: the band around %s was written" % (label, name))
    for name, g in (("qkv", qkv), ("dctx", dctx), ("src_mask", src), ("key_padding", pad)):
        if g is not None and not g.unchanged():
            problems.append("%s: the input %s was written" % (label, name))
    got = dict(ctx=ctx.numpy((T * B, Cc)), lse=lse.numpy((B * H, T)), dsum=dsum.numpy((B * H, T)), dqkv=dq.numpy((T * B, 3 * Cc)))
    r64, r32 = A.refs(case)
    failures, ratios = A.compare(got, r64, r32, factors=FACTORS)
    _report(label, failures, ratios, problems)
    if case["key_padding"] is not None:                # padded keys: the K and V parts of dqkv are exactly +-0
        kv = got["dqkv"].reshape(T, B, 3 * Cc)[:, :, Cc:]
        bad = (kv != 0).any(-1) & (case["key_padding"].T != 0)
        if bad.any():
            problems.append("%s: dK / dV of %d padded keys are not zero, first (t, b) = %s" % (label, int(bad.sum()), np.argwhere(bad)[0]))
    assert not problems, "\n".join(problems)
    return got


# T in {1, 31, 32, 33, 64, 127, 128, 129, 161, 257}, B in {1, 2, 4}, H in {1, 2, 8} (B H = 32 once): every edge of the 32-wide tiles
# and of the deal of key / query tiles to four waves (1, 2, 4, 5, 6 and 9 tiles), with every mask, dropout and dctx kind once.
CASES = {
    "T1": dict(T=1, B=1, H=1),
    "T31-look0-p.1": dict(T=31, B=2, H=2, src=("look", 0), p=0.1),
    "T32-peaked": dict(T=32, B=1, H=8, regime="peaked"),
    # last valid key 31, 32; one valid key at 0; look-ahead combined with padding; the skipped-tile path of the backward pass
    "T33-look3-ragged-p.5": dict(T=33, B=4, H=1, src=("look", 3), pads=[("full",), ("tail", 32), ("tail", 33), ("one", 0)], p=0.5,
                                 dctx="tail5"),
    "T64-random-one-peaked": dict(T=64, B=2, H=1, regime="peaked", src=("random",), pads=[("full",), ("one", 63)]),
    # queries in front of the only / first valid key see nothing under the look-ahead mask; one utterance has no valid key
    "T64-look0-dark-p.1": dict(T=64, B=4, H=2, src=("look", 0), pads=[("dark",), ("one", 63), ("front", 40), ("full",)], p=0.1),
    "T127-random-p.1": dict(T=127, B=1, H=2, src=("random",), p=0.1),
    "T128-BH32-front-dark": dict(T=128, B=4, H=8, pads=[("full",), ("tail", 32), ("front", 33), ("dark",)], dctx="tail5"),
    "T129-look3-ragged-peaked-p.1": dict(T=129, B=2, H=2, regime="peaked", src=("look", 3), pads=[("tail", 128), ("tail", 129)], p=0.1),
    # last valid key 127, 128; a hole; padding in front (first valid key in the second tile); a tile of -0.0 in dctx
    "T161-ragged-hole-front-p.5": dict(T=161, B=4, H=2, pads=[("tail", 128), ("tail", 129), ("hole", 161, 40, 100), ("front", 40)],
                                      p=0.5, dctx="negzero"),
    "T161-one-last-tail5": dict(T=161, B=2, H=1, pads=[("one", 160), ("tail", 20)], dctx="tail5"),
    "T257-look0-hole-lastelem": dict(T=257, B=2, H=1, src=("look", 0), pads=[("full",), ("hole", 257, 70, 200)], dctx="lastelem"),
    "T257-peaked-p.1": dict(T=257, B=1, H=2, regime="peaked", p=0.1),
    "T257-random-ragged-p.5-lastelem": dict(T=257, B=2, H=2, src=("random",), pads=[("tail", 200), ("full",)], p=0.5, dctx="lastelem"),
}


@pytest.mark.parametrize("label", list(CASES))
def test_attention_matches_float64(label):
    run_attention(A.make_case(seed=len(label), **CASES[label]), label)


@pytest.mark.parametrize("T,pads", [(64, None), (128, None), (256, None),
                                    (200, [("hole", 168, 40, 80), ("hole", 200, 100, 172), ("hole", 129, 31, 32)])],
                         ids=["T64", "T128", "T256", "T200-128-valid"])
def test_attention_uniform_rows_are_exact(T, pads):
    """Q = 0, V small integers, a power of two of valid keys per utterance (the tail of the padding and a hole in it leave 128
    of 200): every probability is 1 / n, so ctx = sum(V_valid) / n bit for bit -- a missed or doubled key changes an integer."""
    B, H = 3, 2
    case = A.make_case(T, B, H, pads=pads, seed=1)
    r = np.random.default_rng(T)
    x = case["qkv"].reshape(T, B, 3, H * 64)
    x[:, :, 0] = 0.0
    x[:, :, 2] = r.integers(-8, 9, (T, B, H * 64)).astype(np.float32)
    got = run_attention(case, "uniform-T%d" % T)
    valid = np.ones((B, T), bool) if pads is None else case["key_padding"] == 0
    for b in range(B):
        n = int(valid[b].sum())
        assert n & (n - 1) == 0 and n >= 64
        want = (x[valid[b], b, 2].astype(np.float64).sum(0) / n).astype(np.float32)
        ctx = got["ctx"].reshape(T, B, H * 64)[:, b]
        assert np.array_equal(ctx, np.broadcast_to(want, ctx.shape)), (b, np.argwhere(ctx != want)[0])


def test_attention_one_valid_key_is_exact():
    """Exactly one valid key k* in {0, 31, 32, T - 1}: every probability of it is 1, so ctx[q] = V[k*] bit for bit for every q."""
    T, B, H = 70, 4, 2
    ks = [0, 31, 32, T - 1]
    case = A.make_case(T, B, H, pads=[("one", k) for k in ks], seed=2)
    got = run_attention(case, "one-hot")
    V = case["qkv"].reshape(T, B, 3, H * 64)[:, :, 2]
    ctx = got["ctx"].reshape(T, B, H * 64)
    for b, k in enumerate(ks):
        assert np.array_equal(ctx[:, b].view(np.uint32), np.broadcast_to(V[k, b].view(np.uint32), (T, H * 64))), (b, k)


def test_attention_without_the_padding_shortcuts():
    """This file's attention tests once more in a fresh child process with PK2_ATTN_SKIP_PAD=0 (read once per process): key
    loops that walk every tile and backward kernels that multiply all-zero dctx tiles."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k",
                          "test_attention and not without_the_padding_shortcuts"],
                         env=dict(os.environ, PK2_ATTN_SKIP_PAD="0"), capture_output=True, text=True, timeout=900, cwd=root)
    print(out.stdout[-20000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert "%d passed" % (len(CASES) + 5) in out.stdout and "failed" not in out.stdout, out.stdout[-2000:]


@pytest.mark.parametrize("n", [1, 255, 256, 4096 * 256 + 3])
def test_dropout_is_the_mask_of_dropout_ref(n):
    """pk2_dropout_f32 on ones against keep_mask * scale, bit for bit (n = 4096 * 256 + 3: past the cap of the grid, so some
    threads take a second element), out of place and in place."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    ones = np.ones(n, np.float32)
    for p in (0.0, 0.1, 0.2, 0.5, 0.999):
        for seed in (0, 1, 2 ** 63 - 1):
            mask, scale = dropout_ref.keep_mask(seed, n, p)
            want = np.where(mask, scale, np.float32(0)).astype(np.float32)
            x, y = Guarded(ones), Guarded(n=n)
            _lib.check(L.pk2_dropout_f32(x.ptr, y.ptr, n, p, C.c_uint64(seed), sp))
            z = Guarded(ones, inout=True)
            _lib.check(L.pk2_dropout_f32(z.ptr, z.ptr, n, p, C.c_uint64(seed), sp))
            torch.cuda.synchronize()
            assert y.intact() and z.intact() and x.unchanged(), (p, seed)
            for got in (y.numpy(n), z.numpy(n)):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (p, seed, np.flatnonzero(got != want)[:4])


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["spread", "offset"])
@pytest.mark.parametrize("rows,Cc", [(1, 64), (37, 512), (300, 80), (5, 1000), (513, 1024)])
def test_layernorm_forward_matches_float64(rows, Cc, regime):
    """pk2_layernorm_fwd, res and sum_out both given and both NULL; spread: s ~ N(0.3, 2^2); offset: s ~ 100 + N(0, 1) (the
    variance is a small difference of large numbers for a one-pass formula)."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    r = np.random.default_rng(rows + Cc)
    f32 = lambda v: np.ascontiguousarray(v, np.float32)       # noqa: E731
    x = f32(r.standard_normal((rows, Cc)) * 2 + 0.3 if regime == "spread" else 100 + r.standard_normal((rows, Cc)))
    res, gamma, beta = f32(r.standard_normal((rows, Cc))), f32(r.standard_normal(Cc)), f32(r.standard_normal(Cc))
    problems = []
    for with_res in (True, False):
        label = "layernorm_fwd-%dx%d-%s-%s" % (rows, Cc, regime, "res" if with_res else "nores")
        gx, gr, gg, gb = Guarded(x), Guarded(res) if with_res else None, Guarded(gamma), Guarded(beta)
        s, y = Guarded(n=rows * Cc) if with_res else None, Guarded(n=rows * Cc)
        mean, rstd = Guarded(n=rows), Guarded(n=rows)
        _lib.check(L.pk2_layernorm_fwd(gx.ptr, _opt(gr), gg.ptr, gb.ptr, rows, Cc, 1e-5, _opt(s), y.ptr, mean.ptr, rstd.ptr, sp))
        torch.cuda.synchronize()
        for g in (s, y, mean, rstd):
            if g is not None and not g.intact():
                problems.append("%s: the band around an output was written" % label)
        got = dict(y=y.numpy((rows, Cc)), mean=mean.numpy(rows), rstd=rstd.numpy(rows))
        if with_res:
            got["s"] = s.numpy((rows, Cc))
        refs = [dict(zip(("s", "y", "mean", "rstd"), attention_ref.layernorm_fwd(x, res if with_res else None, gamma, beta,
                                                                                np.float32(1e-5), dt))) for dt in (np.float64, np.float32)]
        failures, ratios = bound_check.compare(got, refs[0], refs[1], ("s", "y", "mean", "rstd"), factors=FACTORS)
        _report(label, failures, ratios, problems)
    assert not problems, "\n".join(problems)


def _mask_kinds(T, B, r):
    """(name, src_mask, key_padding) of the masked-softmax cases at one size."""
    one = lambda a, b: [a, b][:B] if B == 2 else [a]          # noqa: E731
    stack = lambda specs: np.stack([A.padding_row(T, s) for s in specs])        # noqa: E731
    rnd = r.standard_normal((T, T)).astype(np.float32)
    return [("none", None, None), ("look0", A.look_ahead(T, 0), None), ("look3", A.look_ahead(T, 3), None), ("random", rnd, None),
            ("ragged-hole", None, stack(one(("hole", T, T // 4, T // 2), ("tail", T // 2 + 1)))),
            ("look3-front-one", A.look_ahead(T, 3), stack(one(("front", T // 3), ("one", T - 1)))),      # rows with no visible key
            ("random-dark", rnd, stack(one(("dark",), ("full",))))]


@pytest.mark.parametrize("BH", [1, 6])
@pytest.mark.parametrize("T", [1, 33, 255, 256, 257, 600])
def test_masked_softmax_and_its_backward_match_float64(T, BH):
    """pk2_softmax_mask_fwd and pk2_softmax_bwd (both in place) with every kind of mask; a fully masked row comes back all
    zero.  The backward pass is fed the float32 oracle's probabilities."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    B, H = (1, 1) if BH == 1 else (2, 3)
    r = np.random.default_rng(T + BH)
    scores = (3 * r.standard_normal((BH, T, T))).astype(np.float32)
    dP = r.standard_normal((BH, T, T)).astype(np.float32)
    problems = []
    for name, src, pad in _mask_kinds(T, B, r):
        label = "softmax-T%d-BH%d-%s" % (T, BH, name)
        P64, P32 = (attention_ref.softmax_mask_fwd(scores, src, pad, B, H, T, dt) for dt in (np.float64, np.float32))
        gs, gm, gp = Guarded(scores, inout=True, band=2 * T), Guarded(src, band=2 * T) if src is not None else None, \
            Guarded(pad, band=2 * T) if pad is not None else None
        _lib.check(L.pk2_softmax_mask_fwd(gs.ptr, _opt(gm), _opt(gp), B, H, T, sp))
        gP, gd = Guarded(P32, band=2 * T), Guarded(dP, inout=True, band=2 * T)
        _lib.check(L.pk2_softmax_bwd(gP.ptr, gd.ptr, BH, T, sp))
        torch.cuda.synchronize()
        if not (gs.intact() and gd.intact() and gP.unchanged()):
            problems.append("%s: a band or an input was written" % label)
        got = dict(P=gs.numpy((BH, T, T)), dS=gd.numpy((BH, T, T)))
        ref = [dict(P=P, dS=attention_ref.softmax_bwd(P32, dP, dt)) for P, dt in ((P64, np.float64), (P32, np.float32))]
        failures, ratios = bound_check.compare(got, ref[0], ref[1], ("P", "dS"), factors=FACTORS)
        _report(label, failures, ratios, problems)
        dark = ~P64.reshape(B, H, T, T).any(-1)                # rows with no visible key (the oracle's convention)
        if name in ("look3-front-one", "random-dark") and T > 4:
            assert dark.any(), label
        if got["P"].reshape(B, H, T, T)[dark].any():
            problems.append("%s: a fully masked row is not all zero" % label)
    assert not problems, "\n".join(problems)
