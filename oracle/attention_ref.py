"""Multi-head self-attention (head size 64) and the row operators of TransformerAM at the layouts of the C ABI
(include/pk2hip.h: pk2_attention_fwd / _bwd, pk2_layernorm_fwd / _bwd, pk2_softmax_mask_fwd, pk2_softmax_bwd), numpy only.

Written from the operator definitions in the header.  Per (utterance b, head h), with Q, K, V [T, 64] cut out of
qkv[T*B][3*H*64] (row t*B + b; Q | K | V, head h at columns h*64):

    S = Q K^T * scale + src_mask            and S[:, k] = -inf for a padded key k
    P = softmax(S) (plain, with the row maximum subtracted);  lse = log sum exp S
    P_d = P * keep * keep_scale             (dropout on the probabilities; keep[B*H][T][T] from oracle/dropout_ref.py)
    ctx = P_d V
    dP_d = dctx V^T;  dP_dropped = dP_d * keep * keep_scale;  dsum = rowsum(dP_dropped * P)  (= rowsum(dctx * ctx))
    dS = P * (dP_dropped - dsum) * scale;   dQ = dS K;  dK = dS^T Q;  dV = P_d^T dctx

dtype = float64 is the oracle.  dtype = float32 runs the same statements in float32 with numpy's exp / log / sqrt: a model of
a correct float32 implementation (tests/attention_check.py takes the tolerances from its distance to the float64 result on
the same data), not of the kernels' arithmetic.  Its matrix products are written out (_mm): one fused multiply-add per term
of the contracted index, in index order, every partial sum rounded to float32 -- the plain float32 dot product, and what
OpenBLAS's sgemm computes.  numpy's `@` is not used there because its arithmetic depends on the call: for a transposed view
with fewer than about 40 rows it leaves BLAS for a loop of its own that sums in blocks, with a third to a quarter of the
error, so the float32 model -- and with it the bound -- would be another one at T <= 33 than at T >= 48, and another one
from one numpy build to the next.  (oracle/lstm_ref.py still multiplies with `@`: its h W^T products have the same
dependence on the shape -- B rows against a transposed view -- which makes its float32 model tighter at small B, never
looser; it is left as it is so that the LSTM tests' behaviour does not change.)
"""
import numpy as np

HEAD = 64


def _mm(a, b, dtype):
    """a[..., M, K] @ b[..., K, N].  float64: numpy's product.  float32: acc <- fl32(fl64(acc + a[:, k] * b[k, :])) for
    k = 0 .. K-1.  The product of two float32 numbers is exact in float64; the sum is rounded to float64 and then to float32,
    which is a fused multiply-add except where the float64 rounding lands exactly on a float32 tie (double rounding: at most
    half a float32 ulp * 2^-29 further off, and rare) -- tests/test_oracle_attention.py holds it to an exactly rounded chain
    in rational arithmetic."""
    if dtype != np.float32:
        return a @ b
    acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(a.shape[-1]):
        acc = (acc + a64[..., :, k:k + 1] * b64[..., k:k + 1, :]).astype(np.float32)
    return acc


def fwd_bwd(qkv, dctx, T, B, H, scale, src_mask=None, key_padding=None, keep_mask=None, keep_scale=1.0, dtype=np.float64):
    """qkv [T*B, 3*H*64], dctx [T*B, H*64], src_mask [T, T] additive or None, key_padding [B, T] (nonzero = padded) or None,
    keep_mask [B*H, T, T] bool or None -> ctx [T*B, H*64], lse [B*H, T], dsum [B*H, T], dqkv [T*B, 3*H*64].

    A query with no visible key (every key padded, or every score -inf) follows the kernels' convention, not torch's NaN:
    its probabilities are 0, so ctx = 0, lse = -inf, dsum = 0 and it adds nothing to any gradient (its dQ row is 0)."""
    C = H * HEAD
    x = np.asarray(qkv, dtype).reshape(T, B, 3, H, HEAD).transpose(2, 1, 3, 0, 4)      # [3][B][H][T][64]
    Q, K, V = x[0], x[1], x[2]
    dO = np.asarray(dctx, dtype).reshape(T, B, H, HEAD).transpose(1, 2, 0, 3)
    sc = dtype(scale)
    S = _mm(Q, K.transpose(0, 1, 3, 2), dtype) * sc
    if src_mask is not None:
        S = S + np.asarray(src_mask, dtype).reshape(1, 1, T, T)
    if key_padding is not None:
        S = np.where(np.asarray(key_padding).reshape(B, 1, 1, T) != 0, dtype(-np.inf), S)
    m = S.max(-1, keepdims=True)
    dark = np.isneginf(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.exp(S - np.where(dark, dtype(0), m))
        l = e.sum(-1, keepdims=True, dtype=dtype)
        P = np.where(dark, dtype(0), e / l)
        lse = np.where(dark, dtype(-np.inf), m + np.log(l))
    if keep_mask is not None:
        drop = np.asarray(keep_mask).reshape(B, H, T, T).astype(dtype) * dtype(keep_scale)
    else:
        drop = np.ones((1, 1, 1, 1), dtype)
    Pd = P * drop
    ctx = _mm(Pd, V, dtype)
    dPd = _mm(dO, V.transpose(0, 1, 3, 2), dtype) * drop
    dsum = (dPd * P).sum(-1, keepdims=True, dtype=dtype)
    dS = P * (dPd - dsum) * sc
    dQ = _mm(dS, K, dtype)
    dK = _mm(dS.transpose(0, 1, 3, 2), Q, dtype)
    dV = _mm(Pd.transpose(0, 1, 3, 2), dO, dtype)
    dqkv = np.stack([dQ, dK, dV]).transpose(3, 1, 0, 2, 4).reshape(T * B, 3 * C)
    assert ctx.dtype == dtype and dqkv.dtype == dtype and lse.dtype == dtype and dsum.dtype == dtype
    return (np.ascontiguousarray(ctx.transpose(2, 0, 1, 3).reshape(T * B, C)), lse.reshape(B * H, T),
            dsum.reshape(B * H, T), np.ascontiguousarray(dqkv))


def layernorm_fwd(x, res, gamma, beta, eps, dtype=np.float64):
    """s = x + res (res may be None); y = (s - mean) * rstd * gamma + beta with the biased variance -> (s, y, mean, rstd),
    mean / rstd [rows]."""
    s = np.asarray(x, dtype) if res is None else np.asarray(x, dtype) + np.asarray(res, dtype)
    C = s.shape[1]
    mean = s.sum(1, dtype=dtype) / dtype(C)
    d = s - mean[:, None]
    rstd = dtype(1) / np.sqrt((d * d).sum(1, dtype=dtype) / dtype(C) + dtype(eps))
    y = d * rstd[:, None] * np.asarray(gamma, dtype) + np.asarray(beta, dtype)
    return s, y, mean, rstd


def layernorm_bwd(dy, s, mean, rstd, gamma, dtype=np.float64):
    """From the saved s, mean, rstd: ds = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * gamma;
    dgamma = sum_rows dy * xhat; dbeta = sum_rows dy -> (ds, dgamma, dbeta)."""
    dy, s, gamma = np.asarray(dy, dtype), np.asarray(s, dtype), np.asarray(gamma, dtype)
    r = np.asarray(rstd, dtype)[:, None]
    C = s.shape[1]
    xh = (s - np.asarray(mean, dtype)[:, None]) * r
    g = dy * gamma
    ma = g.sum(1, keepdims=True, dtype=dtype) / dtype(C)
    mb = (g * xh).sum(1, keepdims=True, dtype=dtype) / dtype(C)
    return r * (g - ma - xh * mb), (dy * xh).sum(0, dtype=dtype), dy.sum(0, dtype=dtype)


def softmax_mask_fwd(scores, src_mask, key_padding, B, H, T, dtype=np.float64):
    """scores [B*H, T, T] -> softmax over the last axis of scores + src_mask[T, T] with the columns of padded keys
    (key_padding [B, T] nonzero) at -inf; a row with no visible key comes back all zero."""
    S = np.asarray(scores, dtype).reshape(B, H, T, T)
    if src_mask is not None:
        S = S + np.asarray(src_mask, dtype).reshape(1, 1, T, T)
    if key_padding is not None:
        S = np.where(np.asarray(key_padding).reshape(B, 1, 1, T) != 0, dtype(-np.inf), S)
    m = S.max(-1, keepdims=True)
    dark = np.isneginf(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(S - np.where(dark, dtype(0), m))
        P = np.where(dark, dtype(0), e / e.sum(-1, keepdims=True, dtype=dtype))
    return P.reshape(B * H, T, T)


def softmax_bwd(P, dP, dtype=np.float64):
    """dS = P * (dP - rowsum(dP * P))."""
    P, dP = np.asarray(P, dtype), np.asarray(dP, dtype)
    return P * (dP - (dP * P).sum(-1, keepdims=True, dtype=dtype))
