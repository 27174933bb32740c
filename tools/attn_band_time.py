"""Attention core of one TransformerAM layer over a context band: the banded kernels (pk2_attention_band_fwd / _bwd)
against the existing fused kernels given the same band as a dense [T, T] mask, on device events.

Shape: the LF-MMI bench minibatch, B = 4, lengths 146 / 539 / 569 / 159 (key padding behind every utterance's last
frame), at H = 8, d = 64 and at H = 4, d = 128, no dropout.  Bands (left, right, chunk): (-1, 6, 1) = -look_ahead 6,
(64, 6, 1) a sliding window, (64, 0, 32) chunk-wise.  Both legs run alternately in one process, call by call, after a
warm-up of the shape: band forward + backward between two events, then dense forward + backward between two events.  Per
number: the median over --reps calls (at least 50) and the spread = interquartile range of the same calls.  One line per
(head size, band), then one JSON line; `python tools/attn_band_time.py > profiles/attn_band_time.txt`."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import _lib, transformer as tr  # noqa: E402
from pykaldi2_amd.lstm import _p  # noqa: E402

LENS = [146, 539, 569, 159]
HEADS = [(8, 64), (4, 128)]
BANDS = [(-1, 6, 1), (64, 6, 1), (64, 0, 32)]


def time_band(H, d, band, reps, warmup):
    L, sp = _lib.lib(), _lib.stream_ptr()
    B, T, C = len(LENS), max(LENS), H * d
    scale = 1.0 / math.sqrt(d)
    new = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32)  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(B * T + d)
    qkv = torch.randn(T * B, 3 * C, device="cuda", generator=g)
    dcx = torch.randn(T * B, C, device="cuda", generator=g)
    kp = torch.zeros(B, T, dtype=torch.uint8, device="cuda")
    for b, n in enumerate(LENS):
        kp[b, n:] = 1
    mask = tr.BandMask(*band).dense(T).cuda()
    out = [(new(T * B, C), new(B * H, T), new(T * B, 3 * C), new(B * H, T)) for _ in range(2)]

    def banded():
        cx, lse, dqkv, dsum = out[0]
        _lib.check(L.pk2_attention_band_fwd(_p(qkv), T, B, H, d, scale, *band, _p(kp), 0.0, 0, _p(cx), _p(lse), sp))
        _lib.check(L.pk2_attention_band_bwd(_p(qkv), _p(cx), _p(dcx), _p(lse), T, B, H, d, scale, *band, _p(kp), 0.0, 0, _p(dqkv),
                                            _p(dsum), sp))

    def dense():
        cx, lse, dqkv, dsum = out[1]
        _lib.check(L.pk2_attention_fwd(_p(qkv), T, B, H, d, scale, _p(mask), _p(kp), 0.0, 0, _p(cx), _p(lse), sp))
        _lib.check(L.pk2_attention_bwd(_p(qkv), _p(cx), _p(dcx), _p(lse), T, B, H, d, scale, _p(mask), _p(kp), 0.0, 0, _p(dqkv),
                                       _p(dsum), sp))

    def once(timed):
        ev = [torch.cuda.Event(enable_timing=timed) for _ in range(4)]
        ev[0].record(); banded(); ev[1].record()
        ev[2].record(); dense(); ev[3].record()
        torch.cuda.synchronize()
        return (ev[0].elapsed_time(ev[1]) * 1e3, ev[2].elapsed_time(ev[3]) * 1e3) if timed else None

    for _ in range(warmup):
        once(False)
    # the two legs compute the same thing (a wrong kernel is not worth timing)
    for a, b in ((out[0][0], out[1][0]), (out[0][2], out[1][2])):
        assert (a - b).abs().max().item() < 1e-4 * max(1.0, b.abs().max().item())
    t = np.array([once(True) for _ in range(reps)])
    med, iqr = np.median(t, 0), np.percentile(t, 75, 0) - np.percentile(t, 25, 0)
    return dict(band_us=round(float(med[0]), 1), band_spread=round(float(iqr[0]), 1), dense_us=round(float(med[1]), 1),
                dense_spread=round(float(iqr[1]), 1), ratio=round(float(med[1] / med[0]), 2))


def main():
    if not torch.cuda.is_available():
        sys.exit("attn_band_time: no GPU")
    _lib.require_gpu()
    reps = max(50, int(sys.argv[sys.argv.index("--reps") + 1])) if "--reps" in sys.argv else 50
    warmup = max(1, int(sys.argv[sys.argv.index("--warmup") + 1])) if "--warmup" in sys.argv else 10
    result = dict(unit="us", reps=reps, warmup=warmup, B=len(LENS), T=max(LENS), lens=LENS, rows={})
    for H, d in HEADS:
        for band in BANDS:
            r = time_band(H, d, band, reps, warmup)
            result["rows"]["H%d-d%d-%d,%d,%d" % ((H, d) + band)] = r
            print("attn_band_time | H %d d %d | band %s | banded fwd+bwd %.1f (spread %.1f) | dense-mask fwd+bwd %.1f (spread %.1f) us"
                  " | dense / banded %.2f" % (H, d, band, r["band_us"], r["band_spread"], r["dense_us"], r["dense_spread"],
                                             r["ratio"]), flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
