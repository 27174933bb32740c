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

import bound_check
from oracle import lstm_ref

FACTOR = bound_check.FACTOR
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
    """Holds every tensor of `got` (name -> array) to the bound above (tests/bound_check.py, the one implementation of it).
    Returns (failures, ratios): failures is a list of (tensor name, message), empty for a result that passes; ratios[name] =
    error / max(e32, floor), inf for a tensor that is not finite everywhere.  factors: {name: factor} for tensors with a
    bound of their own."""
    return bound_check.compare(got, ref64, ref32, TENSORS, factor=factor, factors=factors)
