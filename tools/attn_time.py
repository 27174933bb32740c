"""Attention core of one TransformerAM layer, fused kernels against the batched-GEMM form, on device events.

Shapes (each with dropout 0 and 0.1 on the probabilities, key padding behind every utterance's last frame):
  a  the LF-MMI bench minibatch at the subsampled rate: B = 4, H = 4, d = 128, lengths 146 / 539 / 569 / 159
  b  the SE shape at 100 fps: B = 8, H = 4, d = 128, lengths between 870 and 1439
  c  H = 8, d = 64 on the lengths of a: the known point
Both forms run alternately in one process, call by call, after a warm-up of the shape: fused forward, dQ, dK / dV (one launch
each, timed separately), then the unfused forward (2 batched GEMMs, masked softmax, dropout) and backward (4 batched GEMMs,
softmax backward, dropout) as transformer.py launches them, each group between two events.  Per number: the median over
--reps calls (at least 50) and the spread = interquartile range of the same calls.  One line per (shape, dropout), then one
JSON line.  `fused_total` against `unfused_total` + `unfused_spread` on shape a decides whether head size 128 is fused by
default (pykaldi2_amd/transformer.py: DEFAULT_FUSED_HEAD_SIZES)."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import _lib, transformer as tr  # noqa: E402
from pykaldi2_amd.lstm import _p  # noqa: E402

SHAPES = [("a", 4, 128, [146, 539, 569, 159]),
          ("b", 4, 128, [1439, 1312, 1207, 1130, 1044, 987, 921, 870]),
          ("c", 8, 64, [146, 539, 569, 159])]


def time_shape(H, d, lens, drop, reps, warmup):
    L, sp = _lib.lib(), _lib.stream_ptr()
    B, T, C = len(lens), max(lens), H * d
    scale = 1.0 / math.sqrt(d)
    dev = "cuda"
    new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(B * T + d)
    qkv = torch.randn(T * B, 3 * C, device=dev, generator=g)
    dcx = torch.randn(T * B, C, device=dev, generator=g)
    kp = torch.zeros(B, T, dtype=torch.uint8, device=dev)
    for b, n in enumerate(lens):
        kp[b, n:] = 1
    seed = 12345
    cx, lse, dqkv, dsum = new(T * B, C), new(B * H, T), new(T * B, 3 * C), new(B * H, T)
    cx0, dqkv0 = new(T * B, C), new(T * B, 3 * C)

    def fused_fwd():
        _lib.check(L.pk2_attention_fwd(_p(qkv), T, B, H, d, scale, None, _p(kp), float(drop), seed, _p(cx), _p(lse), sp))

    def fused_bwd(part):
        _lib.check(L.pk2_attention_bwd_part(part, _p(qkv), _p(cx), _p(dcx), _p(lse), T, B, H, d, scale, None, _p(kp), float(drop),
                                            seed, _p(dqkv), _p(dsum), sp))

    s = {}

    def unfused_fwd():
        Pm = new(B * H, T, T)
        tr._bgemm(0, 1, T, T, d, scale, _p(qkv), B * 3 * C, 3 * C, d, _p(qkv, C), B * 3 * C, 3 * C, d, 0.0, _p(Pm), T,
                  H * T * T, T * T, B, H)
        _lib.check(L.pk2_softmax_mask_fwd(_p(Pm), None, _p(kp), B, H, T, sp))
        Pd = tr._dropout(Pm, drop, seed) if drop > 0 else Pm
        tr._bgemm(0, 0, T, d, T, 1.0, _p(Pd), T, H * T * T, T * T, _p(qkv, 2 * C), B * 3 * C, 3 * C, d, 0.0, _p(cx0),
                  B * C, C, d, B, H)
        s.update(P=Pm, Pd=Pd, seed_attn=seed)

    def unfused_bwd():
        tr._attention_bwd_unfused(L, sp, new, s, qkv, dcx, dqkv0, T, B, C, H, d, drop)

    def once(timed):
        ev = [torch.cuda.Event(enable_timing=timed) for _ in range(7)]
        ev[0].record(); fused_fwd()
        ev[1].record(); fused_bwd(1)
        ev[2].record(); fused_bwd(2)
        ev[3].record()
        ev[4].record(); unfused_fwd()
        ev[5].record(); unfused_bwd()
        ev[6].record()
        torch.cuda.synchronize()
        if not timed:
            return None
        f, q, kv = (ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(3))
        uf, ub = ev[4].elapsed_time(ev[5]) * 1e3, ev[5].elapsed_time(ev[6]) * 1e3
        return f, q, kv, f + q + kv, uf, ub, uf + ub

    for _ in range(warmup):
        once(False)
    # the two forms compute the same thing (a wrong kernel is not worth timing)
    err = (cx - cx0).abs().max().item(), (dqkv - dqkv0).abs().max().item()
    assert err[0] < 1e-4 * max(1.0, cx0.abs().max().item()) and err[1] < 1e-4 * max(1.0, dqkv0.abs().max().item()), err
    t = np.array([once(True) for _ in range(reps)])
    med = np.median(t, 0)
    iqr = np.percentile(t, 75, 0) - np.percentile(t, 25, 0)
    names = ("fused_fwd", "fused_dq", "fused_dkv", "fused_total", "unfused_fwd", "unfused_bwd", "unfused_total")
    out = {n: round(float(m), 1) for n, m in zip(names, med)}
    out.update({n + "_spread": round(float(v), 1) for n, v in zip(names, iqr)})
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("attn_time: no GPU")
    _lib.require_gpu()
    reps = max(50, int(sys.argv[sys.argv.index("--reps") + 1])) if "--reps" in sys.argv else 50
    warmup = max(1, int(sys.argv[sys.argv.index("--warmup") + 1])) if "--warmup" in sys.argv else 10
    result = dict(unit="us", reps=reps, warmup=warmup, shapes={})
    for name, H, d, lens in SHAPES:
        for drop in (0.0, 0.1):
            r = time_shape(H, d, lens, drop, reps, warmup)
            r.update(B=len(lens), H=H, d=d, T=max(lens), dropout=drop)
            result["shapes"]["%s-p%g" % (name, drop)] = r
            print("attn_time | %s | B %d H %d d %d T %d p %g | fused fwd %.1f dq %.1f dkv %.1f total %.1f (spread %.1f) | "
                  "unfused fwd %.1f bwd %.1f total %.1f (spread %.1f) us" %
                  (name, len(lens), H, d, max(lens), drop, r["fused_fwd"], r["fused_dq"], r["fused_dkv"], r["fused_total"],
                   r["fused_total_spread"], r["unfused_fwd"], r["unfused_bwd"], r["unfused_total"], r["unfused_total_spread"]),
                  flush=True)
    a = [result["shapes"]["a-p%g" % p] for p in (0.0, 0.1)]
    result["head128_fused_by_default"] = all(r["fused_total"] <= r["unfused_total"] + r["unfused_total_spread"] for r in a)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
