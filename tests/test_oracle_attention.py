"""oracle/attention_ref.py and oracle/dropout_ref.py against torch float64 autograd, and the bound of
tests/attention_check.py -- what tests/test_gpu_attention.py holds the kernels to -- against float32 results that carry one
planted fault each: the bound has to reject every one of them, and to pass the float32 oracle itself with ratio <= 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_check as A
from oracle import attention_ref, dropout_ref

HOLE = [("full",), ("hole", 37, 9, 21)]
RAGGED = [("tail", 33), ("full",)]


def _torch_attention(case, keep, kscale):
    T, B, H = case["T"], case["B"], case["H"]
    qkv = torch.from_numpy(case["qkv"]).double().requires_grad_(True)
    x = qkv.reshape(T, B, 3, H, 64).permute(2, 1, 3, 0, 4)
    s = x[0] @ x[1].transpose(-1, -2) * case["scale"]
    if case["src_mask"] is not None:
        s = s + torch.from_numpy(case["src_mask"]).double()
    if case["key_padding"] is not None:
        s = s.masked_fill(torch.from_numpy(case["key_padding"]).bool().reshape(B, 1, 1, T), float("-inf"))
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * torch.from_numpy(keep.reshape(B, H, T, T)).double() * float(kscale)
    ctx = (p @ x[2]).permute(2, 0, 1, 3).reshape(T * B, H * 64)
    dctx = torch.from_numpy(case["dctx"]).double()
    ctx.backward(dctx)
    return dict(ctx=ctx.detach().numpy(), lse=torch.logsumexp(s, -1).reshape(B * H, T).detach().numpy(), dqkv=qkv.grad.numpy(),
                dsum=(dctx * ctx.detach()).reshape(T, B, H, 64).sum(-1).permute(1, 2, 0).reshape(B * H, T).numpy())


@pytest.mark.parametrize("kw", [dict(T=40, B=2, H=2, src=("look", 0), pads=RAGGED),
                                dict(T=40, B=2, H=1, src=("look", 3), p=0.1),
                                dict(T=45, B=2, H=2, pads=HOLE, p=0.5, regime="peaked"),
                                dict(T=33, B=1, H=3, src=("random",), p=0.1),
                                dict(T=70, B=2, H=2, src=("random",), pads=[("front", 35), ("one", 69)], dctx="lastelem"),
                                dict(T=1, B=1, H=1)],
                         ids=["look0-ragged", "look3-dropout", "hole-dropout-peaked", "random-dropout", "random-front-one", "T1"])
def test_float64_oracle_equals_torch_autograd(kw):
    case = A.make_case(seed=3, **kw)
    T, B, H = case["T"], case["B"], case["H"]
    keep, kscale = (dropout_ref.keep_mask(case["seed"], B * H * T * T, case["p"]) if case["p"] > 0 else (None, 1.0))
    want = _torch_attention(case, keep, kscale)
    got = A.refs(case)[0]
    for name in A.TENSORS:
        assert got[name].dtype == np.float64 and got[name].shape == want[name].shape
        err = np.abs(got[name] - want[name]).max()
        assert err <= 1e-12, (name, err)


def test_a_query_without_a_visible_key_gives_zero_and_minus_infinity():
    """The kernels' convention, not torch's NaN: utterance 1 has no valid key, and under the look-ahead mask the queries in
    front of utterance 0's only valid key (30) see nothing either."""
    case = A.make_case(41, 2, 2, src=("look", 0), pads=[("one", 30), ("dark",)], p=0.1, seed=5)
    for ref in A.refs(case):
        ctx, dqkv = ref["ctx"].reshape(41, 2, 128), ref["dqkv"].reshape(41, 2, 3, 128)
        lse, dsum = ref["lse"].reshape(2, 2, 41), ref["dsum"].reshape(2, 2, 41)
        assert np.isneginf(lse[1]).all() and np.isneginf(lse[0, :, :30]).all() and np.isfinite(lse[0, :, 30:]).all()
        assert not ctx[:, 1].any() and not ctx[:30, 0].any() and not dsum[1].any() and not dsum[0, :, :30].any()
        assert not dqkv[:, 1].any() and not dqkv[:30, 0, 0].any()
        assert np.isfinite(ctx).all() and np.isfinite(dqkv).all() and np.isfinite(dsum).all()
        assert dqkv[30, 0, 2].any()                                # (one visible key: P = 1, so dS = 0 and only dV is not zero)
        assert not np.delete(dqkv[:, 0, 1:], 30, 0).any()          # padded keys: dK = dV = 0


@pytest.mark.parametrize("rows,C,with_res", [(1, 64, True), (37, 512, False), (5, 1000, True)])
def test_layernorm_oracle_equals_torch_autograd(rows, C, with_res):
    r = np.random.default_rng(rows + C)
    x, res = r.standard_normal((rows, C)) * 2 + 0.3, r.standard_normal((rows, C)) if with_res else None
    gamma, beta, dy = r.standard_normal(C), r.standard_normal(C), r.standard_normal((rows, C))
    s, y, mean, rstd = attention_ref.layernorm_fwd(x, res, gamma, beta, 1e-5)
    ds, dgamma, dbeta = attention_ref.layernorm_bwd(dy, s, mean, rstd, gamma)
    st = torch.from_numpy(x if res is None else x + res).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    yt = F.layer_norm(st, (C,), gt, bt, 1e-5)
    yt.backward(torch.from_numpy(dy))
    assert np.array_equal(s, st.detach().numpy())
    for got, want in ((y, yt.detach()), (mean, st.detach().mean(1)), (rstd, 1 / torch.sqrt(st.detach().var(1, unbiased=False) + 1e-5)),
                      (ds, st.grad), (dgamma, gt.grad), (dbeta, bt.grad)):
        assert got.dtype == np.float64 and np.abs(got - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize("T,B,H", [(1, 1, 1), (33, 2, 3)])
def test_softmax_oracles_equal_torch_autograd(T, B, H):
    r = np.random.default_rng(T)
    scores, dP = r.standard_normal((B * H, T, T)) * 3, r.standard_normal((B * H, T, T))
    src = A.look_ahead(T, 0) + r.standard_normal((T, T)).astype(np.float32)
    pad = np.stack([A.padding_row(T, ("tail", max(1, T - 2 * b))) for b in range(B)])
    P = attention_ref.softmax_mask_fwd(scores, src, pad, B, H, T)
    st = torch.from_numpy(scores).reshape(B, H, T, T).requires_grad_(True)
    Pt = torch.softmax((st + torch.from_numpy(src).double()).masked_fill(torch.from_numpy(pad).bool().reshape(B, 1, 1, T), float("-inf")), -1)
    Pt.backward(torch.from_numpy(dP).reshape(B, H, T, T))
    assert np.abs(P - Pt.detach().numpy().reshape(B * H, T, T)).max() <= 1e-12
    assert np.abs(attention_ref.softmax_bwd(P, dP) - st.grad.numpy().reshape(B * H, T, T)).max() <= 1e-12
    dark = attention_ref.softmax_mask_fwd(scores, None, np.ones((B, T), np.uint8), B, H, T, np.float32)
    assert dark.dtype == np.float32 and not dark.any()


def test_keep_mask_is_a_pure_function_with_the_right_rate():
    n = 1 << 20
    for p in (0.1, 0.5, 0.999):
        a, scale = dropout_ref.keep_mask(7, n, p)
        b, _ = dropout_ref.keep_mask(7, n, p)
        c, _ = dropout_ref.keep_mask(8, n, p)
        assert a.dtype == np.bool_ and a.shape == (n,) and np.array_equal(a, b) and not np.array_equal(a, c)
        keep = 1.0 - float(np.float32(p))
        assert scale.dtype == np.float32 and scale == np.float32(1.0 / keep)
        assert abs(a.mean() - keep) <= 4 * np.sqrt(keep * (1 - keep) / n), (p, a.mean())
        assert np.array_equal(a[:1000], dropout_ref.keep_mask(7, 1000, p)[0])       # element i does not depend on n
    assert dropout_ref.keep_mask(2 ** 63 - 1, 100, 0.0)[0].all() and dropout_ref.keep_mask(0, 100, 0.0)[1] == 1.0
    # one value worked by hand from the definition, in Python integers
    M, seed, i = (1 << 64) - 1, 12345, 77
    z = (seed * 0xD1342543DE82EF95 + i + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    assert bool(dropout_ref.keep_mask(seed, 78, 0.5)[0][77]) == ((z >> 32) < (1 << 31))


# ---------------------------------------------------------------------------------------------------------------------
# the bound against planted faults
# ---------------------------------------------------------------------------------------------------------------------
FAULT_CASE = dict(T=45, B=2, H=2, src=("random",), pads=[("full",), ("tail", 40)], p=0.1, seed=9)


def _result(case, fault):
    """The float32 oracle's result with one fault planted (None: none)."""
    T, B, H = case["T"], case["B"], case["H"]
    C = H * 64
    keep, kscale = dropout_ref.keep_mask(case["seed"], B * H * T * T, case["p"])
    keep = keep.reshape(B * H, T, T)
    src, pad = case["src_mask"], case["key_padding"].copy()
    if fault in ("key32", "keyT-1"):                   # one key of a tile boundary dropped
        pad[:, 32 if fault == "key32" else T - 1] = 1
    elif fault == "dropout_transposed":                # the dropout mask indexed [k][q]
        keep = np.ascontiguousarray(keep.transpose(0, 2, 1))
    elif fault == "mask_row_q+1":
        src = src[np.minimum(np.arange(T) + 1, T - 1)]
    elif fault == "padded_key_let_through":
        pad[1, 42] = 0
    ctx, lse, dsum, dqkv = attention_ref.fwd_bwd(case["qkv"], case["dctx"], T, B, H, case["scale"], src, pad, keep, kscale, np.float32)
    if fault == "dk_without_scale":
        dqkv = dqkv.copy()
        dqkv[:, C:2 * C] /= np.float32(case["scale"])
    elif fault == "dsum_before_division":              # rowsum(dO * O) with O not yet divided by l = exp(lse - max)
        x = case["qkv"].reshape(T, B, 3, H, 64).transpose(2, 1, 3, 0, 4)
        s = x[0] @ x[1].transpose(0, 1, 3, 2) * np.float32(case["scale"]) + src
        s = np.where(pad.reshape(B, 1, 1, T) != 0, -np.inf, s)
        dsum = dsum * np.exp(lse - s.max(-1).reshape(B * H, T)).astype(np.float32)
    return dict(ctx=ctx, lse=lse, dsum=dsum, dqkv=dqkv)


@pytest.mark.parametrize("kw", [FAULT_CASE, dict(T=64, B=1, H=2, regime="peaked", src=("look", 0), seed=2),
                                dict(T=41, B=2, H=2, src=("look", 0), pads=[("one", 30), ("dark",)], p=0.1, seed=5)],
                         ids=["fault-case", "peaked-look0", "dark-rows"])
def test_the_float32_oracle_passes_with_ratio_at_most_one(kw):
    case = A.make_case(**kw)
    r64, r32 = A.refs(case)
    failures, ratios = A.compare(r32, r64, r32)
    assert failures == [] and set(ratios) == set(A.TENSORS) and max(ratios.values()) <= 1.0, (failures, ratios)


@pytest.mark.parametrize("fault,caught_in", [("key32", "ctx"), ("keyT-1", "ctx"), ("dropout_transposed", "ctx"),
                                             ("mask_row_q+1", "ctx"), ("dk_without_scale", "dqkv"),
                                             ("dsum_before_division", "dsum"), ("padded_key_let_through", "ctx")])
def test_the_bound_rejects_a_planted_fault(fault, caught_in):
    case = A.make_case(**FAULT_CASE)
    r64, r32 = A.refs(case)
    assert A.compare(_result(case, None), r64, r32)[0] == []
    failures, ratios = A.compare(_result(case, fault), r64, r32)
    assert caught_in in [name for name, _ in failures], (fault, ratios)
    assert ratios[caught_in] > 100 * A.FACTOR, (fault, ratios)


def test_the_bound_rejects_unwritten_elements_and_a_finite_value_for_minus_infinity():
    case = A.make_case(41, 2, 2, src=("look", 0), pads=[("one", 30), ("dark",)], seed=5)
    r64, r32 = A.refs(case)
    got = {k: v.copy() for k, v in r32.items()}
    got["lse"][3, 7] = -1e30                       # float64 oracle: -inf
    got["dqkv"][5, 100] = np.nan
    got["ctx"][0, 0] = np.inf
    failures, ratios = A.compare(got, r64, r32)
    assert sorted(n for n, _ in failures) == ["ctx", "dqkv", "lse"] and ratios["dsum"] <= 1.0
    got = {k: v.copy() for k, v in r32.items()}
    got["lse"][0, 35] = -np.inf                    # float64 oracle: finite
    assert [n for n, _ in A.compare(got, r64, r32)[0]] == ["lse"]


def _round_to_float32(x):
    """The float32 nearest to the Fraction x, ties to even (normal range only)."""
    from fractions import Fraction
    if x == 0:
        return Fraction(0)
    e = abs(x).numerator.bit_length() - abs(x).denominator.bit_length()
    if Fraction(2) ** e > abs(x):
        e -= 1
    assert Fraction(2) ** e <= abs(x) < Fraction(2) ** (e + 1) and -126 <= e <= 127
    quantum = Fraction(2) ** (e - 23)
    return round(x / quantum) * quantum             # round(Fraction) rounds halves to even


def test_the_float32_products_are_an_in_order_chain_at_every_size():
    """attention_ref._mm in float32 against a chain of exactly rounded fused multiply-adds in rational arithmetic (acc <-
    fl32(acc + a_k b_k), k in index order), and the same bits whatever the shape or the memory layout of the operands
    (numpy's `@` sums transposed views with few rows another way than large ones, which would make the float32 error model
    -- and the bound -- depend on T); in float64 it is numpy's product."""
    from fractions import Fraction
    r = np.random.default_rng(4)
    a = (3 * r.standard_normal((4, 64))).astype(np.float32)
    b = (3 * r.standard_normal((5, 64))).astype(np.float32)
    got = attention_ref._mm(a, b.T, np.float32)
    for i in range(4):
        for j in range(5):
            acc = Fraction(0)
            for k in range(64):
                acc = _round_to_float32(acc + Fraction(float(a[i, k])) * Fraction(float(b[j, k])))
            assert Fraction(float(got[i, j])) == acc, (i, j)
    for T in (3, 32, 70):
        a = (3 * r.standard_normal((2, T, 64))).astype(np.float32)
        b = (3 * r.standard_normal((2, T, 64))).astype(np.float32)
        got = attention_ref._mm(a, b.transpose(0, 2, 1), np.float32)
        assert got.dtype == np.float32
        assert np.array_equal(got, attention_ref._mm(np.ascontiguousarray(a), np.ascontiguousarray(b.transpose(0, 2, 1)), np.float32))
        for n in range(2):
            for i in range(0, T, 7):          # a row of the stack computed alone: the same chain, another shape
                assert np.array_equal(got[n, i], attention_ref._mm(a[n, i:i + 1], b[n].T, np.float32)[0])
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        assert np.array_equal(attention_ref._mm(a64, b64.transpose(0, 2, 1), np.float64), a64 @ b64.transpose(0, 2, 1))
