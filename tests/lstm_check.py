"""Data and comparison shared by tests/test_oracle_lstm.py (CPU) and tests/test_gpu_lstm_layer.py (device): what a result of
one LSTM layer is held to, and the two data regimes it is held to it on.  Plain module, no GPU, no pytest.

The bound of tensor X in a case is taken from a correct float32 implementation on that very data, never from the kernels:

    e32(X)   = max |X_float32-oracle - X_float64-oracle|
    floor(X) = 2^-23 * max |X_float64-oracle|
    max |X_result - X_float64-oracle|  <=  FACTOR * max(e32(X), floor(X)),     FACTOR = 4

(4: another summation order of the K = H products and two 1-ulp hardware approximations per nonlinearity where libm is
rounded to half an ulp -- each worth a small factor, none an order of magnitude.)  No element is excluded, and a NaN or an
inf anywhere in a result is a failure whatever the data.
"""
import numpy as np

from oracle import lstm_ref

FACTOR = 4.0
TENSORS = ("y", "gates", "cells", "dgx", "dbias_ih", "dbias_hh")


def make_case(B, T, H, D, regime, with_bias, seed):
    """Inputs of one layer, rounded to float32: whh, bhh ~ U(+-1/sqrt(H)) as torch initialises them (bhh None without bias);
    linear: gx, dy ~ N(0, 1); saturated: gx ~ N(0, 8^2) with 1 % of the entries replaced by +-U(40, 120) -- gates at exactly
    0 and 1 in float32, exp2 overflowing inside both nonlinearities -- and the weights NOT scaled up (the recurrence stays
    contractive, so float32 tracks float64 and a tolerance means something)."""
    r = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    whh = r.uniform(-k, k, (D, 4 * H, H))
    bhh = r.uniform(-k, k, (D, 4 * H))
    gx = r.standard_normal((T, B, D * 4 * H))
    if regime == "saturated":
        gx *= 8.0
        m = r.random(gx.shape) < 0.01
        gx[m] = np.where(r.random(int(m.sum())) < 0.5, -1.0, 1.0) * r.uniform(40.0, 120.0, int(m.sum()))
    else:
        assert regime == "linear", regime
    dy = r.standard_normal((T, B, D * H))
    f32 = lambda v: np.ascontiguousarray(v, np.float32)
    return dict(gx=f32(gx), whh=f32(whh), bhh=f32(bhh) if with_bias else None, dy=f32(dy), B=B, T=T, H=H, D=D)


def forward_refs(case):
    """(float64 oracle, float32 oracle) of the forward pass: dicts y / gates / cells."""
    out = []
    for dt in (np.float64, np.float32):
        y, gates, cells = lstm_ref.layer_fwd(case["gx"], case["whh"], case["bhh"], dt)
        out.append(dict(y=y, gates=gates, cells=cells))
    return out


def backward_refs(case, gates, cells, dbias_ih0=None, dbias_hh0=None):
    """(float64 oracle, float32 oracle) of the backward pass from the given float32 activations: dict dgx, and -- when the
    values the accumulators held before the call are given -- dbias_ih / dbias_hh = those values + the sum of dgx."""
    out = []
    for dt in (np.float64, np.float32):
        dgx, dbias = lstm_ref.layer_bwd(case["dy"], case["whh"], gates, cells, dt)
        ref = dict(dgx=dgx)
        if dbias_ih0 is not None:
            ref["dbias_ih"] = np.asarray(dbias_ih0, dt) + dbias
            ref["dbias_hh"] = np.asarray(dbias_hh0, dt) + dbias
        out.append(ref)
    return out


def compare(got, ref64, ref32, factor=FACTOR, factors=None):
    """Holds every tensor of `got` (name -> array) to the bound above.  Returns (failures, ratios): failures is a list of
    (tensor name, message), empty for a result that passes; ratios[name] = error / max(e32, floor), inf for a tensor that is
    not finite everywhere.  factors: {name: factor} for tensors with a bound of their own."""
    failures, ratios = [], {}
    for name in TENSORS:
        if name not in got:
            continue
        x = np.asarray(got[name])
        want, model = ref64[name], ref32[name]
        if x.shape != want.shape:
            failures.append((name, "%s: shape %s, expected %s" % (name, x.shape, want.shape)))
            ratios[name] = float("inf")
            continue
        bad = ~np.isfinite(x)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            failures.append((name, "%s: %d of %d elements not finite (unwritten or NaN / inf), first at %s"
                             % (name, int(bad.sum()), x.size, at)))
            ratios[name] = float("inf")
            continue
        e32 = float(np.abs(model.astype(np.float64) - want).max())
        floor = 2.0 ** -23 * float(np.abs(want).max())
        unit = max(e32, floor)
        diff = np.abs(x.astype(np.float64) - want)
        err = float(diff.max())
        ratios[name] = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
        f = (factors or {}).get(name, factor)
        if not err <= f * unit:
            at = tuple(int(v) for v in np.unravel_index(int(diff.argmax()), diff.shape))
            failures.append((name, "%s: error %.3g at %s (got %.9g, float64 %.9g) > %g * max(e32 %.3g, floor %.3g): ratio %.1f"
                             % (name, err, at, float(x[at]), float(want[at]), f, e32, floor, ratios[name])))
    return failures, ratios
