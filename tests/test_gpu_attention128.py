"""The fused attention kernels at head size 128 (csrc/attention128.hip) through the C ABI, against the numpy oracle
oracle/attention_ref.py with its module constant HEAD set to 128 (scale = 128 ** -0.5), held to the bound of
tests/bound_check.py unchanged:

    max |X - X_float64-oracle|  <=  4 * max(e32(X), 2^-23 * max |X_float64-oracle|)

The cases are the CASES table of tests/test_gpu_attention.py (same specs, same seeds).  The head-128 kernels keep the
32-wide (query x key) tiles and the deal of key / query tiles to four waves of the head-64 kernels, so the edges of the
tiling are the ones that table was written for: T in {1, 31, 32, 33, 64, 127, 128, 129, 161, 257} = 1, 2, 4, 5, 6 and 9
tiles; no further T is needed.  Memory hygiene as there: outputs pre-filled with NaN between bands of a bit pattern that
must survive, inputs between bands of NaN and unchanged afterwards, dK / dV of padded keys exactly +-0.  One line per
(case, tensor) is printed: attention128_ratio | case | tensor | ratio.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_check as A
import test_gpu_attention as T64
from oracle import attention_ref
from pykaldi2_amd import _lib

pytestmark = pytest.mark.gpu

HEAD = 128
# tensor -> factor, for a tensor that needs more than bound_check.FACTOR: only with the arithmetic step that costs it named here.
FACTORS = {}
Guarded, _opt = T64.Guarded, T64._opt


@pytest.fixture(autouse=True)
def head128(monkeypatch):
    """make_case / refs at head size 128: both modules read their HEAD when called."""
    monkeypatch.setattr(attention_ref, "HEAD", HEAD)
    monkeypatch.setattr(A, "HEAD", HEAD)


def run_attention(case, label):
    """tests/test_gpu_attention.py: run_attention at head size 128 -- forward, then backward on the kernel's own ctx / lse;
    memory hygiene, the bound, exact zeros at padded keys.  Returns the device results."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    T, B, H = case["T"], case["B"], case["H"]
    Cc = H * HEAD
    assert case["qkv"].shape == (T * B, 3 * Cc) and case["scale"] == HEAD ** -0.5
    qkv, dctx = Guarded(case["qkv"], band=2 * 3 * Cc), Guarded(case["dctx"], band=2 * Cc)
    src = Guarded(case["src_mask"], band=2 * T) if case["src_mask"] is not None else None
    pad = Guarded(case["key_padding"], band=2 * T) if case["key_padding"] is not None else None
    ctx, dq = Guarded(n=T * B * Cc, band=2 * Cc), Guarded(n=T * B * 3 * Cc, band=2 * 3 * Cc)
    lse, dsum = Guarded(n=B * H * T, band=2 * T), Guarded(n=B * H * T, band=2 * T)
    seed = C.c_uint64(case["seed"])
    _lib.check(L.pk2_attention_fwd(qkv.ptr, T, B, H, HEAD, case["scale"], _opt(src), _opt(pad), case["p"], seed, ctx.ptr, lse.ptr, sp))
    torch.cuda.synchronize()
    _lib.check(L.pk2_attention_bwd(qkv.ptr, ctx.ptr, dctx.ptr, lse.ptr, T, B, H, HEAD, case["scale"], _opt(src), _opt(pad), case["p"],
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
    for name, r in ratios.items():
        print("attention128_ratio | %s | %s | %.3f" % (label, name, r))
    problems += ["%s: %s" % (label, msg) for _, msg in failures]
    if case["key_padding"] is not None:                # padded keys: the K and V parts of dqkv are exactly +-0
        kv = got["dqkv"].reshape(T, B, 3 * Cc)[:, :, Cc:]
        bad = (kv != 0).any(-1) & (case["key_padding"].T != 0)
        if bad.any():
            problems.append("%s: dK / dV of %d padded keys are not zero, first (t, b) = %s" % (label, int(bad.sum()), np.argwhere(bad)[0]))
    assert not problems, "\n".join(problems)
    return got


@pytest.mark.parametrize("label", list(T64.CASES))
def test_attention128_matches_float64(label):
    run_attention(A.make_case(seed=len(label), **T64.CASES[label]), label)


@pytest.mark.parametrize("T,pads", [(64, None), (128, None), (256, None),
                                    (200, [("hole", 168, 40, 80), ("hole", 200, 100, 172), ("hole", 129, 31, 32)])],
                         ids=["T64", "T128", "T256", "T200-128-valid"])
def test_attention128_uniform_rows_are_exact(T, pads):
    """Q = 0, V small integers, a power of two of valid keys per utterance: every probability is 1 / n, so ctx =
    sum(V_valid) / n bit for bit -- a missed or doubled key changes an integer."""
    B, H = 3, 2
    case = A.make_case(T, B, H, pads=pads, seed=1)
    r = np.random.default_rng(T)
    x = case["qkv"].reshape(T, B, 3, H * HEAD)
    x[:, :, 0] = 0.0
    x[:, :, 2] = r.integers(-8, 9, (T, B, H * HEAD)).astype(np.float32)
    got = run_attention(case, "uniform-T%d" % T)
    valid = np.ones((B, T), bool) if pads is None else case["key_padding"] == 0
    for b in range(B):
        n = int(valid[b].sum())
        assert n & (n - 1) == 0 and n >= 64
        want = (x[valid[b], b, 2].astype(np.float64).sum(0) / n).astype(np.float32)
        ctx = got["ctx"].reshape(T, B, H * HEAD)[:, b]
        assert np.array_equal(ctx, np.broadcast_to(want, ctx.shape)), (b, np.argwhere(ctx != want)[0])


def test_attention128_one_valid_key_is_exact():
    """Exactly one valid key k* in {0, 31, 32, T - 1}: every probability of it is 1, so ctx[q] = V[k*] bit for bit for every q."""
    T, B, H = 70, 4, 2
    ks = [0, 31, 32, T - 1]
    case = A.make_case(T, B, H, pads=[("one", k) for k in ks], seed=2)
    got = run_attention(case, "one-hot")
    V = case["qkv"].reshape(T, B, 3, H * HEAD)[:, :, 2]
    ctx = got["ctx"].reshape(T, B, H * HEAD)
    for b, k in enumerate(ks):
        assert np.array_equal(ctx[:, b].view(np.uint32), np.broadcast_to(V[k, b].view(np.uint32), (T, H * HEAD))), (b, k)


def test_attention128_uses_all_128_dimensions():
    """Q and K are non-zero only in dimensions 64..127 of each head and V differs between the two halves; H = 2, so head 1
    starts at column 128.  A kernel that reads 64 columns per head sees Q = K = 0: uniform rows, far outside the bound."""
    T, B, H = 33, 2, 2
    case = A.make_case(T, B, H, seed=3)
    x = case["qkv"].reshape(T, B, 3, H, HEAD)
    x[:, :, :2, :, :64] = 0.0
    x[:, :, 2, :, 64:] += 3.0
    run_attention(case, "upper-half")
    r64, _ = A.refs(case)
    rows = r64["ctx"].reshape(T, B, H, HEAD)
    assert np.abs(rows - rows.mean(0)).max() > 0.1          # (the case can tell: the true rows are far from uniform)


_SKIP_SNIPPET = r"""
import ctypes, sys, numpy as np, torch
sys.path.insert(0, %r)
from pykaldi2_amd import _lib
L = _lib.lib(); sp = _lib.stream_ptr()
p = lambda t: ctypes.c_void_p(t.data_ptr())
T, B, H, d = 200, 4, 2, 128
scale = 128 ** -0.5
C = H * d
g = torch.Generator(device="cuda").manual_seed(7)
qkv = torch.randn(T, B, 3 * C, device="cuda", generator=g)
lens = [200, 33, 1, 150]
kpm = torch.zeros(B, T, dtype=torch.uint8, device="cuda")
for b, n in enumerate(lens):
    kpm[b, n:] = 1
kpm[3, 40:100] = 1                                 # padding with a hole behind it
dctx = torch.randn(T, B, C, device="cuda", generator=g)
for b, n in enumerate(lens):
    dctx[min(T, n + 5):, b] = 0.0                  # no loss term reaches frames far behind an utterance's end
ctx = torch.empty(T, B, C, device="cuda"); lse = torch.empty(B * H, T, device="cuda")
_lib.check(L.pk2_attention_fwd(p(qkv), T, B, H, d, scale, None, p(kpm), 0.1, 99, p(ctx), p(lse), sp))
dqkv = torch.full((T, B, 3 * C), float("nan"), device="cuda"); dsum = torch.empty(B * H, T, device="cuda")
_lib.check(L.pk2_attention_bwd(p(qkv), p(ctx), p(dctx), p(lse), T, B, H, d, scale, None, p(kpm), 0.1, 99, p(dqkv), p(dsum), sp))
torch.cuda.synchronize()
np.savez(sys.argv[1], ctx=ctx.cpu().numpy(), lse=lse.cpu().numpy(), dqkv=dqkv.cpu().numpy())
"""


def test_attention128_padding_shortcuts_change_no_bit(tmp_path):
    """PK2_ATTN_SKIP_PAD = 0, 1 and 3 (read once per process, hence three child processes): ctx, lse and dqkv equal bit for
    bit (ragged lengths, a one-key utterance, padding with a hole, dropout on the probabilities).  A child that fails ends
    the test; nothing is run again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for mode in ("0", "1", "3"):
        out = str(tmp_path / ("attn128_%s.npz" % mode))
        env = dict(os.environ, PK2_ATTN_SKIP_PAD=mode)
        r = subprocess.run([sys.executable, "-c", _SKIP_SNIPPET % root, out], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])
        outs.append(np.load(out))
    assert np.isfinite(outs[0]["dqkv"]).all()       # every element written
    for other in outs[1:]:
        for k in ("ctx", "lse", "dqkv"):
            a, b = outs[0][k], other[k]
            assert np.isfinite(b[np.isfinite(a)]).all()
            assert np.array_equal(a, b, equal_nan=True), k
        assert np.isfinite(other["dqkv"]).all()


@pytest.mark.parametrize("d", [32, 96])
def test_other_head_sizes_are_still_refused(d):
    L, sp = _lib.lib(), _lib.stream_ptr()
    T, B, H = 8, 1, 1
    qkv = torch.zeros(T * B, 3 * H * d, device="cuda")
    ctx, lse = torch.zeros(T * B, H * d, device="cuda"), torch.zeros(B * H, T, device="cuda")
    dqkv, dsum = torch.zeros_like(qkv), torch.zeros_like(lse)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    with pytest.raises(_lib.Pk2Error, match="head size"):
        _lib.check(L.pk2_attention_fwd(p(qkv), T, B, H, d, d ** -0.5, None, None, 0.0, C.c_uint64(0), p(ctx), p(lse), sp))
    with pytest.raises(_lib.Pk2Error, match="head size"):
        _lib.check(L.pk2_attention_bwd(p(qkv), p(ctx), p(ctx), p(lse), T, B, H, d, d ** -0.5, None, None, 0.0, C.c_uint64(0),
                                       p(dqkv), p(dsum), sp))
    torch.cuda.synchronize()
