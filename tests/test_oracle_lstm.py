"""The float64 LSTM layer oracle (oracle/lstm_ref.py) against torch.nn.LSTM in float64, and the comparison of
tests/lstm_check.py -- what tests/test_gpu_lstm_layer.py holds the kernels to -- against float32 results that carry one
defect each: it has to report every one of them, on the right tensor, and accept the clean float32 result."""
import numpy as np
import pytest
import torch

import lstm_check
from oracle import lstm_ref


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,T,H,D", [(3, 1, 16, 1), (2, 1, 8, 2), (4, 7, 16, 1), (3, 9, 24, 2)])
def test_oracle_matches_torch_float64(B, T, H, D, with_bias):
    """y against torch.nn.LSTM on x with gx = x W_ih^T + b_ih formed outside in float64; d gx = gx.grad through a
    torch.nn.LSTM whose input IS gx (W_ih selects the direction's 4H columns, b_ih = 0) with the same W_hh, b_hh."""
    torch.manual_seed(B * 100 + T)
    Din, G = 5, 4 * H
    m = torch.nn.LSTM(Din, H, 1, bidirectional=D == 2).double()
    sfx = ["", "_reverse"][:D]
    if not with_bias:
        with torch.no_grad():
            for s in sfx:
                getattr(m, "bias_hh_l0" + s).zero_()
    x = torch.randn(T, B, Din, dtype=torch.float64)
    gx = torch.cat([x @ getattr(m, "weight_ih_l0" + s).T + getattr(m, "bias_ih_l0" + s) for s in sfx], -1).detach()
    whh = np.stack([getattr(m, "weight_hh_l0" + s).detach().numpy() for s in sfx])
    bhh = np.stack([getattr(m, "bias_hh_l0" + s).detach().numpy() for s in sfx]) if with_bias else None
    want_y = m(x)[0].detach().numpy()
    y, gates, cells = lstm_ref.layer_fwd(gx.numpy(), whh, bhh)
    assert y.dtype == np.float64 and gates.shape == (D, T, B, G) and cells.shape == (D, T, B, H)
    assert np.abs(y - want_y).max() <= 1e-12 * max(1.0, np.abs(want_y).max())

    m2 = torch.nn.LSTM(D * G, H, 1, bidirectional=D == 2).double()
    with torch.no_grad():
        for d, s in enumerate(sfx):
            sel = torch.zeros(G, D * G, dtype=torch.float64)
            sel[:, d * G:(d + 1) * G] = torch.eye(G, dtype=torch.float64)
            getattr(m2, "weight_ih_l0" + s).copy_(sel)
            getattr(m2, "bias_ih_l0" + s).zero_()
            getattr(m2, "weight_hh_l0" + s).copy_(getattr(m, "weight_hh_l0" + s))
            getattr(m2, "bias_hh_l0" + s).copy_(getattr(m, "bias_hh_l0" + s))
    gx.requires_grad_()
    y2 = m2(gx)[0]
    assert np.abs(y2.detach().numpy() - want_y).max() <= 1e-12 * max(1.0, np.abs(want_y).max())
    dy = torch.randn(T, B, D * H, dtype=torch.float64)
    (y2 * dy).sum().backward()
    want_dgx = gx.grad.numpy()
    dgx, dbias = lstm_ref.layer_bwd(dy.numpy(), whh, gates, cells)
    assert np.abs(dgx - want_dgx).max() <= 1e-12 * max(1.0, np.abs(want_dgx).max())
    want_db = want_dgx.reshape(T * B, D, G).sum(0)
    assert dbias.shape == (D, G) and np.abs(dbias - want_db).max() <= 1e-12 * max(1.0, np.abs(want_db).max())
    # the gates and cells the backward pass is given are the forward pass's: i, f, o in (0, 1), g in (-1, 1), c = f c' + i g
    i, f, g = gates[..., :H], gates[..., H:2 * H], gates[..., 2 * H:3 * H]
    for d in range(D):
        ts = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for n, t in enumerate(ts):
            cp = cells[d, ts[n - 1]] if n else 0.0
            assert np.abs(cells[d, t] - (f[d, t] * cp + i[d, t] * g[d, t])).max() <= 1e-15


# ---- float32 results with one defect each -----------------------------------------------------------------------------
def _sig(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def _fwd32(case, defect=None):
    """oracle/lstm_ref.layer_fwd in float32 into NaN-filled buffers, with the named defect."""
    dt = np.float32
    gx, whh = case["gx"], case["whh"]
    T, B, H, D = case["T"], case["B"], case["H"], case["D"]
    G = 4 * H
    bhh = np.zeros((D, G), dt) if case["bhh"] is None else case["bhh"].copy()
    if defect == "bhh_gate_dropped":
        bhh[D - 1, H:2 * H] = 0                      # the forget gate's recurrent bias of the reverse direction
    y, gates, cells = (np.full(s, np.nan, dt) for s in ((T, B, D * H), (D, T, B, G), (D, T, B, H)))
    for d in range(D):
        h, c = np.zeros((B, H), dt), np.zeros((B, H), dt)
        ts = range(T) if d == 0 or defect == "reverse_from_t0" else range(T - 1, -1, -1)
        for n, t in enumerate(ts):
            pre = gx[t, :, d * G:(d + 1) * G] + h @ whh[d].T + bhh[d]
            i, f, o, g = _sig(pre[:, :H]), _sig(pre[:, H:2 * H]), _sig(pre[:, 3 * H:]), np.tanh(pre[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            rows = B - 1 if defect == "row_unwritten" and n == T - 1 else B
            y[t, :rows, d * H:(d + 1) * H] = h[:rows]
            gates[d, t] = np.concatenate([i, f, g, o], 1)
            cells[d, t] = c
    return dict(y=y, gates=gates, cells=cells)


def _bwd32(case, gates, cells, dbias_ih0, dbias_hh0, defect=None, stale_dc=None):
    dt = np.float32
    dy, whh = case["dy"], case["whh"]
    T, B, H, D = case["T"], case["B"], case["H"], case["D"]
    G = 4 * H
    dgx = np.full((T, B, D * G), np.nan, dt)
    summed = np.zeros((T, B, D * G), dt)            # what the bias gradient sums: every row, written out or not
    last_dc = np.zeros((D, B, H), dt)
    for d in range(D):
        ts = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        dh = np.zeros((B, H), dt)
        dc = np.zeros((B, H), dt) if stale_dc is None else stale_dc[d].copy()
        for n in range(T - 1, -1, -1):
            t = ts[n]
            cprev = cells[d, ts[n - 1]] if n > 0 else np.zeros((B, H), dt)
            if defect == "ct_for_cprev":
                cprev = cells[d, t]
            i, f, g, o = (gates[d, t][:, k * H:(k + 1) * H] for k in range(4))
            tc = np.tanh(cells[d, t])
            dht = dy[t, :, d * H:(d + 1) * H] + dh
            dcv = dc + dht * o * (1 - tc * tc)
            dg = np.concatenate([dcv * g * i * (1 - i), dcv * cprev * f * (1 - f), dcv * i * (1 - g * g), dht * tc * o * (1 - o)], 1)
            rows = B - 1 if defect == "row_unwritten" and n == 0 else B
            dgx[t, :rows, d * G:(d + 1) * G] = dg[:rows]
            summed[t, :, d * G:(d + 1) * G] = dg
            dc = dcv * f
            dh = dg @ whh[d]
            if defect == "dh_unit_left_out":
                dh[:, H - 1] = 0
        last_dc[d] = dc
    if defect == "dc_carried_over" and stale_dc is None:      # the scratch's dc of the call before is this call's first dc
        return _bwd32(case, gates, cells, dbias_ih0, dbias_hh0, None, last_dc)
    dbias = summed.reshape(T * B, D, G).sum(0, dtype=dt)
    if defect == "dbias_assigned":
        return dict(dgx=dgx, dbias_ih=dbias, dbias_hh=dbias)
    return dict(dgx=dgx, dbias_ih=dbias_ih0 + dbias, dbias_hh=dbias_hh0 + dbias)


FORWARD = {"y", "gates", "cells"}
BACKWARD = {"dgx", "dbias_ih", "dbias_hh"}
# defect -> (tensors that must be reported, tensors that may be)
DEFECTS = {
    "bhh_gate_dropped": ({"gates", "cells", "y"}, FORWARD),
    "reverse_from_t0": ({"y", "gates", "cells"}, FORWARD),
    "ct_for_cprev": ({"dgx"}, BACKWARD),
    "dc_carried_over": ({"dgx"}, BACKWARD),
    "row_unwritten": ({"y", "dgx"}, {"y", "dgx"}),
    "dbias_assigned": ({"dbias_ih", "dbias_hh"}, {"dbias_ih", "dbias_hh"}),
    "dh_unit_left_out": ({"dgx"}, BACKWARD),
}


def _run(case, defect):
    """What the device helper does, on the float32 model: forward, then backward from the float64 oracle's activations
    rounded to float32, accumulators pre-filled with different random values."""
    f64, f32 = lstm_check.forward_refs(case)
    got = _fwd32(case, defect)
    r = np.random.default_rng(5)
    D, G = case["D"], 4 * case["H"]
    b_ih0, b_hh0 = r.standard_normal((D, G)).astype(np.float32), r.standard_normal((D, G)).astype(np.float32)
    gates, cells = f64["gates"].astype(np.float32), f64["cells"].astype(np.float32)
    b64, b32 = lstm_check.backward_refs(case, gates, cells, b_ih0, b_hh0)
    got.update(_bwd32(case, gates, cells, b_ih0, b_hh0, defect))
    f64.update(b64)
    f32.update(b32)
    return lstm_check.compare(got, f64, f32)


@pytest.mark.parametrize("regime", ["linear", "saturated"])
@pytest.mark.parametrize("with_bias", [True, False])
def test_clean_float32_result_is_accepted(regime, with_bias):
    for B, T, H, D in [(3, 5, 64, 2), (1, 1, 64, 1), (5, 40, 128, 2)]:
        failures, ratios = _run(lstm_check.make_case(B, T, H, D, regime, with_bias, seed=B + T), None)
        assert failures == [], failures
        assert set(ratios) == set(lstm_check.TENSORS) and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("regime", ["linear", "saturated"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_comparison_reports_every_defect_on_its_tensor(defect, regime):
    case = lstm_check.make_case(3, 6, 64, 2, regime, True, seed=11)
    failures, ratios = _run(case, defect)
    named = {name for name, _ in failures}
    must, may = DEFECTS[defect]
    assert must <= named, (defect, must - named, ratios)
    assert named <= may, (defect, named - may, failures)
    for name, msg in failures:
        assert msg.startswith(name + ":")
    if defect == "row_unwritten":     # row B-1 of the last step: y at t = 0 of the reverse direction (and t = T-1 of the
        msgs = dict(failures)         # forward one), dgx at t = 0 of the forward direction (and t = T-1 of the reverse one)
        assert "128 of 2304" in msgs["y"] and "first at (0, 2, 64)" in msgs["y"], msgs
        assert "512 of 9216" in msgs["dgx"] and "first at (0, 2, 0)" in msgs["dgx"], msgs
