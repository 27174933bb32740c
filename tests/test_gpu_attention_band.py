"""The banded attention kernels (csrc/attention_band.hip) through the C ABI, against the float64 oracle
oracle/attention_ref.py given the band as a dense src_mask, held to the bound of tests/bound_check.py unchanged
(attention_check.compare: ctx, lse, dsum, dqkv; lse exactly -inf where the oracle's is).  Head size 128 as in
tests/test_gpu_attention128.py: the oracle's HEAD set to 128.  B = 2, H = 2; T = 33 is one tile and a row, 97 four tiles
(one workgroup) with a ragged end, 161 six tiles: a second, partial workgroup and walks longer than the ring.  Outputs are
NaN between canary bands before every call."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_check as A
import test_gpu_attention as T64
from oracle import attention_ref
from pykaldi2_amd import _lib

pytestmark = pytest.mark.gpu
Guarded, _opt = T64.Guarded, T64._opt
B, H = 2, 2


def band_mask(T, left, right, chunk):
    q, k = np.arange(T)[:, None], np.arange(T)[None, :]
    seen = ((left < 0) | (k >= q // chunk * chunk - left)) & ((right < 0) | (k <= q // chunk * chunk + chunk - 1 + right))
    return np.where(seen, 0.0, -np.inf).astype(np.float32)


def set_head(monkeypatch, head):
    monkeypatch.setattr(attention_ref, "HEAD", head)
    monkeypatch.setattr(A, "HEAD", head)


def run_band(case, band, head):
    """Forward, then backward on the kernels' own ctx / lse -> the four tensors; the canaries around them must survive."""
    L, sp = _lib.lib(), _lib.stream_ptr()
    T, Bc, Hc, Cc = case["T"], case["B"], case["H"], case["H"] * head
    qkv, dctx = Guarded(case["qkv"], band=2 * 3 * Cc), Guarded(case["dctx"], band=2 * Cc)
    pad = Guarded(case["key_padding"], band=2 * T) if case["key_padding"] is not None else None
    ctx, dq = Guarded(n=T * Bc * Cc, band=2 * Cc), Guarded(n=T * Bc * 3 * Cc, band=2 * 3 * Cc)
    lse, dsum = Guarded(n=Bc * Hc * T, band=2 * T), Guarded(n=Bc * Hc * T, band=2 * T)
    seed = C.c_uint64(case["seed"])
    _lib.check(L.pk2_attention_band_fwd(qkv.ptr, T, Bc, Hc, head, case["scale"], *band, _opt(pad), case["p"], seed, ctx.ptr,
                                        lse.ptr, sp))
    _lib.check(L.pk2_attention_band_bwd(qkv.ptr, ctx.ptr, dctx.ptr, lse.ptr, T, Bc, Hc, head, case["scale"], *band, _opt(pad),
                                        case["p"], seed, dq.ptr, dsum.ptr, sp))
    torch.cuda.synchronize()
    for name, g in (("ctx", ctx), ("lse", lse), ("dqkv", dq), ("dsum", dsum)):
        assert g.intact(), "the band around %s was written" % name
    return dict(ctx=ctx.numpy((T * Bc, Cc)), lse=lse.numpy((Bc * Hc, T)), dsum=dsum.numpy((Bc * Hc, T)),
                dqkv=dq.numpy((T * Bc, 3 * Cc)))


TAIL = [("tail", 140), ("tail", 75)]           # both ends inside a tile: the band of the last valid queries reaches into padding
TAIL97 = [("tail", 40), ("tail", 87)]
FRONT = [("front", 40), ("full",)]             # with left = 5 the queries below 35 of utterance 0 see no key
DARK = [("dark",), ("full",)]
CASES = [  # head, T, (left, right, chunk), pads, dropout, regime
    (64, 33, (0, 0, 1), None, 0.0, "linear"), (64, 97, (-1, 0, 1), None, 0.0, "linear"),
    (64, 161, (-1, 3, 1), None, 0.0, "linear"), (64, 161, (-1, 3, 1), None, 0.0, "peaked"),
    (64, 97, (5, -1, 1), None, 0.0, "linear"), (64, 161, (31, 0, 1), None, 0.0, "linear"),
    (64, 97, (32, 0, 1), None, 0.0, "linear"), (64, 161, (33, 1, 1), None, 0.0, "linear"),
    (64, 161, (-1, -1, 1), None, 0.0, "linear"), (64, 97, (16, 0, 8), None, 0.0, "linear"),
    (64, 161, (32, 0, 32), None, 0.0, "linear"), (64, 161, (20, 2, 24), None, 0.0, "linear"),
    (64, 33, (20, 2, 24), None, 0.0, "linear"), (64, 161, (33, 1, 1), TAIL, 0.0, "linear"),
    (64, 161, (20, 2, 24), TAIL, 0.0, "linear"), (64, 97, (5, 0, 1), FRONT, 0.0, "linear"),
    (64, 97, (16, 0, 8), DARK, 0.0, "linear"), (64, 161, (31, 0, 1), None, 0.1, "linear"),
    (64, 97, (20, 2, 24), TAIL97, 0.1, "linear"),
    (128, 33, (0, 0, 1), None, 0.0, "linear"), (128, 97, (-1, 0, 1), None, 0.0, "linear"),
    (128, 161, (-1, -1, 1), None, 0.0, "linear"), (128, 161, (20, 2, 24), None, 0.0, "peaked"),
    (128, 161, (33, 1, 1), TAIL, 0.0, "linear"), (128, 97, (5, 0, 1), FRONT, 0.0, "linear"),
    (128, 97, (32, 0, 32), DARK, 0.0, "linear"), (128, 161, (31, 0, 1), None, 0.1, "linear"),
    (128, 97, (16, 0, 8), TAIL97, 0.1, "linear"),
]


@pytest.mark.parametrize("head,T,band,pads,p,regime", CASES)
def test_band_matches_float64(head, T, band, pads, p, regime, monkeypatch):
    set_head(monkeypatch, head)
    case = A.make_case(T, B, H, regime=regime, pads=pads, p=p, seed=T + band[0])
    got = run_band(case, band, head)
    if band != (-1, -1, 1):                          # (no restriction: the oracle with no mask at all)
        case["src_mask"] = band_mask(T, *band)
    r64, r32 = A.refs(case)
    failures, ratios = A.compare(got, r64, r32)
    for name, r in ratios.items():
        print("attention_band_ratio | d%d T%d %s %s p%g %s | %s | %.3f" % (head, T, band, pads, p, regime, name, r))
    assert not failures, "\n".join(msg for _, msg in failures)
    if pads in (FRONT, DARK):                        # the case has what it is there for: queries with no visible key
        assert np.isneginf(r64["lse"]).any() and not np.isneginf(r64["lse"]).all()


@pytest.mark.parametrize("head,band", [(64, (20, 2, 24)), (128, (33, 1, 1))])
def test_band_is_deterministic_alone_and_in_a_batch(head, band, monkeypatch):
    """The same call twice, and utterance 0 alone against utterance 0 beside another one: identical bits (dropout on: the draws
    of utterance 0 are indexed the same in both)."""
    set_head(monkeypatch, head)
    T, Cc = 161, H * head
    case = A.make_case(T, B, H, pads=TAIL, p=0.1, seed=5)
    first, second = run_band(case, band, head), run_band(case, band, head)
    alone = dict(case, B=1, qkv=np.ascontiguousarray(case["qkv"].reshape(T, B, 3 * Cc)[:, 0]),
                 dctx=np.ascontiguousarray(case["dctx"].reshape(T, B, Cc)[:, 0]), key_padding=case["key_padding"][:1])
    single = run_band(alone, band, head)
    for name, shape in (("ctx", (T, B, Cc)), ("dqkv", (T, B, 3 * Cc))):
        assert np.array_equal(first[name], second[name], equal_nan=True), name
        assert np.array_equal(first[name].reshape(shape)[:, 0], single[name].reshape(T, -1), equal_nan=True), name
    for name in ("lse", "dsum"):
        assert np.array_equal(first[name], second[name], equal_nan=True), name
        assert np.array_equal(first[name][:H], single[name], equal_nan=True), name


@pytest.mark.parametrize("head,left,right,chunk", [(64, 0, 0, 0), (64, -2, 0, 1), (64, 0, -2, 1), (32, 0, 0, 1)])
def test_band_refuses_on_the_host(head, left, right, chunk):
    L, sp = _lib.lib(), _lib.stream_ptr()
    T = 8
    qkv = torch.zeros(T, 3 * head, device="cuda")
    ctx, lse = torch.zeros(T, head, device="cuda"), torch.zeros(1, T, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    with pytest.raises(_lib.Pk2Error):
        _lib.check(L.pk2_attention_band_fwd(p(qkv), T, 1, 1, head, 1.0, left, right, chunk, None, 0.0, C.c_uint64(0), p(ctx),
                                            p(lse), sp))
    with pytest.raises(_lib.Pk2Error):
        _lib.check(L.pk2_attention_band_bwd(p(qkv), p(ctx), p(ctx), p(lse), T, 1, 1, head, 1.0, left, right, chunk, None, 0.0,
                                            C.c_uint64(0), p(qkv), p(lse), sp))
    with pytest.raises(_lib.Pk2Error):
        _lib.check(L.pk2_attention_band_fwd(None, T, 1, 1, 64, 1.0, 0, 0, 1, None, 0.0, C.c_uint64(0), p(ctx), p(lse), sp))
    torch.cuda.synchronize()
