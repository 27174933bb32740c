"""Data and comparison shared by tests/test_oracle_attention.py (CPU) and tests/test_gpu_attention.py (device): what a result
of the fused attention and of the TransformerAM row kernels is held to (tests/bound_check.py, the bound of the LSTM tests,
unchanged), and the cases it is held to it on.  Plain module, no GPU, no pytest."""
import numpy as np

import bound_check
from oracle import attention_ref, dropout_ref

FACTOR = bound_check.FACTOR
TENSORS = ("ctx", "lse", "dsum", "dqkv")
HEAD = 64


def compare(got, ref64, ref32, tensors=TENSORS, factor=FACTOR, factors=None):
    """bound_check.compare over `tensors`, all of which `got` has to hold; where the float64 lse is -inf the result must be
    exactly -inf."""
    missing = [name for name in tensors if name not in got]
    assert not missing, "no result for %s" % missing
    return bound_check.compare(got, ref64, ref32, tensors, factor=factor, factors=factors, neg_inf=("lse",))


def look_ahead(T, look):
    """tril(diagonal=look) as 0 / -inf: query q sees the keys k <= q + look."""
    q, k = np.arange(T)[:, None], np.arange(T)[None, :]
    return np.where(k <= q + look, 0.0, -np.inf).astype(np.float32)


def padding_row(T, spec):
    """One utterance's key padding [T] uint8 (1 = padded) from ("full",) | ("tail", n): keys [0, n) valid |
    ("one", k): key k only | ("hole", n, a, b): [0, n) valid but [a, b) | ("front", a): [a, T) valid | ("dark",): no valid key."""
    pad = np.ones(T, np.uint8)
    kind = spec[0]
    if kind == "full":
        pad[:] = 0
    elif kind == "tail":
        pad[:spec[1]] = 0
    elif kind == "one":
        pad[spec[1] % T] = 0
    elif kind == "hole":
        pad[:spec[1]] = 0
        pad[spec[2]:spec[3]] = 1
    elif kind == "front":
        pad[spec[1]:] = 0
    else:
        assert kind == "dark", spec
    return pad


def make_case(T, B, H, regime="linear", src=None, pads=None, p=0.0, dctx="dense", seed=0):
    """Inputs of one attention call, rounded to float32.  linear: qkv, dctx ~ N(0, 1); peaked: Q and K scaled by 3, so the
    scores are ~ N(0, 9^2) and a few keys carry each row.  src: None | ("look", n) | ("random",): a finite additive mask
    ~ N(0, 1).  pads: None or one padding_row spec per utterance.  dctx: dense | tail5: zero from 5 frames behind every
    utterance's last valid key on | negzero: the second query tile of utterance 0 is -0.0 | lastelem: the second query tile
    of every utterance is zero but for the last element of its last row."""
    r = np.random.default_rng(1000003 * seed + 10007 * T + 101 * B + H)
    C = H * HEAD
    qkv = r.standard_normal((T, B, 3 * C))
    if regime == "peaked":
        qkv[:, :, :2 * C] *= 3.0
    else:
        assert regime == "linear", regime
    d = r.standard_normal((T, B, C))
    src_mask = None
    if src is not None:
        src_mask = look_ahead(T, src[1]) if src[0] == "look" else r.standard_normal((T, T)).astype(np.float32)
    key_padding = None
    if pads is not None:
        assert len(pads) == B
        key_padding = np.stack([padding_row(T, s) for s in pads])
    if dctx == "tail5":
        for b in range(B):
            valid = np.flatnonzero(key_padding[b] == 0)
            d[(valid[-1] + 1 if valid.size else 0) + 5:, b] = 0.0
    elif dctx == "negzero":
        d[32:64, 0] = -0.0
    elif dctx == "lastelem":
        d[32:64] = 0.0
        d[min(T, 64) - 1, :, C - 1] = 1.75
    else:
        assert dctx == "dense", dctx
    f32 = lambda v: np.ascontiguousarray(v, np.float32)       # noqa: E731
    return dict(qkv=f32(qkv).reshape(T * B, 3 * C), dctx=f32(d).reshape(T * B, C), T=T, B=B, H=H, scale=HEAD ** -0.5,
                src_mask=src_mask, key_padding=key_padding, p=float(p), seed=int(977 + seed))


def refs(case):
    """(float64 oracle, float32 oracle) of a case: dicts ctx / lse / dsum / dqkv.  The keep mask is dropout_ref's."""
    T, B, H = case["T"], case["B"], case["H"]
    keep, kscale = None, 1.0
    if case["p"] > 0:
        keep, kscale = dropout_ref.keep_mask(case["seed"], B * H * T * T, case["p"])
        keep = keep.reshape(B * H, T, T)
    out = []
    for dt in (np.float64, np.float32):
        v = attention_ref.fwd_bwd(case["qkv"], case["dctx"], T, B, H, case["scale"], case["src_mask"], case["key_padding"],
                                  keep, kscale, dt)
        out.append(dict(zip(TENSORS, v)))
    return out
