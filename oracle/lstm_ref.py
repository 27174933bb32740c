"""One (bi)directional LSTM layer at the layouts of the C ABI (include/pk2hip.h: pk2_lstm_layer_fwd / _bwd), numpy only.

Written from the equations in the header: gate order i, f, g, o; h0 = c0 = 0; direction 0 walks t = 0 .. T-1, direction 1
walks t = T-1 .. 0; all activations time-major.

    pre_t = gx[t, :, d] + h_{t-1} W_hh[d]^T + b_hh[d]
    i, f, o = sigmoid(pre_i), sigmoid(pre_f), sigmoid(pre_o);  g = tanh(pre_g)
    c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)

dtype = float64 is the oracle.  dtype = float32 runs the same statements in float32 with numpy's exp / tanh: a model of a
correct float32 implementation (the tolerances of tests/test_gpu_lstm_layer.py are taken from its distance to the float64
result on the same data), not of the kernels' arithmetic.
"""
import numpy as np


def _sigmoid(x):
    with np.errstate(over="ignore"):          # exp(-x) = inf for x < -88 (float32): 1 / inf = 0, the right limit
        return 1 / (1 + np.exp(-x))


def _order(T, d):
    """Frames of direction d in processing order."""
    return list(range(T)) if d == 0 else list(range(T - 1, -1, -1))


def layer_fwd(gx, whh, bhh=None, dtype=np.float64):
    """gx [T, B, D*4H], whh [D, 4H, H], bhh [D, 4H] or None -> y [T, B, D*H], gates [D, T, B, 4H], cells [D, T, B, H]."""
    gx, whh = np.asarray(gx, dtype), np.asarray(whh, dtype)
    T, B, _ = gx.shape
    D, G, H = whh.shape
    assert G == 4 * H and gx.shape[2] == D * G and D in (1, 2)
    bhh = np.zeros((D, G), dtype) if bhh is None else np.asarray(bhh, dtype)
    y, gates, cells = np.zeros((T, B, D * H), dtype), np.zeros((D, T, B, G), dtype), np.zeros((D, T, B, H), dtype)
    for d in range(D):
        h, c = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        for t in _order(T, d):
            pre = gx[t, :, d * G:(d + 1) * G] + h @ whh[d].T + bhh[d]
            i, f, o = _sigmoid(pre[:, :H]), _sigmoid(pre[:, H:2 * H]), _sigmoid(pre[:, 3 * H:])
            g = np.tanh(pre[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            y[t, :, d * H:(d + 1) * H] = h
            gates[d, t] = np.concatenate([i, f, g, o], 1)
            cells[d, t] = c
    return y, gates, cells


def layer_bwd(dy, whh, gates, cells, dtype=np.float64):
    """dy [T, B, D*H] and the forward pass's gates / cells -> dgx [T, B, D*4H] (gradient wrt the pre-activations),
    dbias [D, 4H] = sum of dgx over t and b."""
    dy, whh, gates, cells = (np.asarray(v, dtype) for v in (dy, whh, gates, cells))
    D, T, B, G = gates.shape
    H = G // 4
    dgx = np.zeros((T, B, D * G), dtype)
    one = dtype(1)
    for d in range(D):
        ts = _order(T, d)
        dh, dc = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
        for n in range(T - 1, -1, -1):
            t = ts[n]
            cprev = cells[d, ts[n - 1]] if n > 0 else np.zeros((B, H), dtype)
            i, f, g, o = (gates[d, t][:, k * H:(k + 1) * H] for k in range(4))
            tc = np.tanh(cells[d, t])
            dht = dy[t, :, d * H:(d + 1) * H] + dh
            dcv = dc + dht * o * (one - tc * tc)
            dg = np.concatenate([dcv * g * i * (one - i), dcv * cprev * f * (one - f), dcv * i * (one - g * g),
                                 dht * tc * o * (one - o)], 1)
            dgx[t, :, d * G:(d + 1) * G] = dg
            dc = dcv * f
            dh = dg @ whh[d]
    dbias = dgx.reshape(T * B, D, G).sum(0, dtype=dtype)
    return dgx, dbias
