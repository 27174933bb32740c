"""float64 restatement of Kaldi's LinearResample / ResampleWaveform for the resampler's tests and for
tools/resample_time.py.  numpy only.

  g = gcd(fi, fo), iu = fi / g, ou = fo / g, cutoff = 0.99 * 0.5 * min(fi, fo), ww = num_zeros / (2 cutoff)
  phase p: t = p / fo, first[p] = ceil((t - ww) fi), last[p] = floor((t + ww) fi)
  w[p][j] = f(dt) h(dt) / fi at dt = (first[p] + j) / fi - t,  f = sin(2 pi cutoff dt) / (pi dt)  (2 cutoff at 0),
  h = 0.5 (1 + cos(2 pi cutoff / num_zeros dt)) inside |dt| < ww, else 0
  y[u ou + p] = gain * sum_j w[p][j] x[first[p] + u iu + j], x = 0 outside [0, n_in);  n_out = ceil(n_in fo / fi)
"""
import math

import numpy as np

RATIOS = [(14400, 16000), (17600, 16000), (16000, 8000), (8000, 16000), (48000, 16000), (15217, 16000)]


def plan(fi, fo, cutoff=None, num_zeros=6):
    """(iu, ou, first (ou) int64, taps (ou) int64, weights (ou, max_taps) float64, zero beyond taps[p])."""
    fi, fo = int(fi), int(fo)
    g = math.gcd(fi, fo)
    iu, ou = fi // g, fo // g
    if fi == fo:
        return 1, 1, np.zeros(1, np.int64), np.ones(1, np.int64), np.ones((1, 1))
    cutoff = 0.99 * 0.5 * min(fi, fo) if cutoff is None else float(cutoff)
    ww = num_zeros / (2.0 * cutoff)
    first, rows = np.zeros(ou, np.int64), []
    for p in range(ou):
        t = p / float(fo)
        lo, hi = math.ceil((t - ww) * fi), math.floor((t + ww) * fi)
        first[p] = lo
        dt = np.arange(lo, hi + 1, dtype=np.float64) / fi - t
        h = np.where(np.abs(dt) < ww, 0.5 * (1.0 + np.cos(2.0 * np.pi * cutoff / num_zeros * dt)), 0.0)
        safe = np.where(dt != 0.0, dt, 1.0)
        f = np.where(dt != 0.0, np.sin(2.0 * np.pi * cutoff * safe) / (np.pi * safe), 2.0 * cutoff)
        rows.append(f * h / fi)
    taps = np.array([len(r) for r in rows], np.int64)
    w = np.zeros((ou, int(taps.max())))
    for p, r in enumerate(rows):
        w[p, :len(r)] = r
    return iu, ou, first, taps, w


def num_output(n_in, fi, fo):
    return -(-int(n_in) * int(fo) // int(fi))


def apply(x, iu, ou, first, taps, w, n_out, gain=1.0):
    """The sum with the given tables in float64: (y (n_out), B (n_out)) with B[k] = sum_j |w_j x_j|."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    w = np.asarray(w, np.float64)
    k = np.arange(n_out, dtype=np.int64)
    u, p = k // ou, k % ou
    start = np.asarray(first, np.int64)[p] + u * iu
    y, B = np.zeros(n_out), np.zeros(n_out)
    for j in range(w.shape[1]):
        idx = start + j
        ok = (j < np.asarray(taps)[p]) & (idx >= 0) & (idx < n)
        term = np.where(ok, w[p, j] * x[np.clip(idx, 0, n - 1)], 0.0)
        y += term
        B += np.abs(term)
    return gain * y, B


def resample(x, fi, fo, gain=1.0, cutoff=None, num_zeros=6):
    iu, ou, first, taps, w = plan(fi, fo, cutoff, num_zeros)
    return apply(x, iu, ou, first, taps, w, num_output(len(x), fi, fo), gain)[0]
