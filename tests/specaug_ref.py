"""numpy restatement of pk2_spec_augment (include/pk2hip.h) from a host plan: the warp as a float64 lerp, exact
copies everywhere else, then the masks in output coordinates."""
import numpy as np

MAX_FREQ, MAX_TIME, BINS = 4, 16, 80
STRIDE = 2 + 2 * MAX_FREQ + 2 * MAX_TIME
FREQ0, TIME0 = 2, 2 + 2 * MAX_FREQ


def plan_row(c=0, d=0, freq=(), time=()):
    row = np.zeros(STRIDE, np.int32)
    row[0], row[1] = c, d
    for k, (a, b) in enumerate(freq):
        row[FREQ0 + 2 * k], row[FREQ0 + 2 * k + 1] = a, b
    for k, (a, b) in enumerate(time):
        row[TIME0 + 2 * k], row[TIME0 + 2 * k + 1] = a, b
    return row


def warp_sources(T, c, d):
    """Per output frame: (i, i1, r, den) -- out[t] = in[i] when r == 0, else in[i] + r / den (in[i1] - in[i])."""
    src = []
    for t in range(T):
        if c == d:
            src.append((t, t, 0, 1))
            continue
        if t <= d:
            base, num, den = 0, t * c, d
        else:
            base, num, den = c, (t - d) * (T - 1 - c), T - 1 - d
        i = min(max(base + num // den, 0), T - 1)
        src.append((i, min(i + 1, T - 1), num % den, den))
    return src


def spec_augment(feats, frames, plan, fill=0.0, warp=True):
    """feats: float32 [sum(frames), 80].  Returns (bits uint32, exact bool, out float64, bound float64), each [rows, 80].
    `exact` marks the elements that are copies or fill: there `bits` is the answer's bit pattern (moved as integers, so
    -0.0, denormals and NaN payloads survive).  Elsewhere `out` is the float64 lerp and `bound` its |a| + |b|."""
    feats = np.ascontiguousarray(feats, np.float32)
    xbits = feats.view(np.uint32)
    fill_bits = np.float32(fill).view(np.uint32)
    bits = np.zeros(feats.shape, np.uint32)
    out = np.zeros(feats.shape, np.float64)
    exact = np.ones(feats.shape, bool)
    bound = np.zeros(feats.shape, np.float64)
    r0 = 0
    for T, row in zip(frames, plan):
        x, xb = feats[r0:r0 + T], xbits[r0:r0 + T]
        y, yb, e, bd = out[r0:r0 + T], bits[r0:r0 + T], exact[r0:r0 + T], bound[r0:r0 + T]
        c, d = (int(row[0]), int(row[1])) if warp else (0, 0)
        for t, (i, i1, r, den) in enumerate(warp_sources(T, c, d)):
            if r == 0:
                yb[t] = xb[i]
            else:
                a, b = x[i].astype(np.float64), x[i1].astype(np.float64)
                y[t] = a + (r / den) * (b - a)
                e[t] = False
                bd[t] = np.abs(a) + np.abs(b)
        for k in range(MAX_FREQ):
            a, b = int(row[FREQ0 + 2 * k]), int(row[FREQ0 + 2 * k + 1])
            yb[:, a:b], e[:, a:b] = fill_bits, True
        for k in range(MAX_TIME):
            a, b = int(row[TIME0 + 2 * k]), int(row[TIME0 + 2 * k + 1])
            yb[a:b], e[a:b] = fill_bits, True
        r0 += T
    return bits, exact, out, bound
