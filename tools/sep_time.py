"""Device time of the blind separation front end, written to profiles/sep_time.txt: C = 7 channels, fft 512 /
frame 400 / shift 160, four utterances of 4.4 / 16.2 / 17.1 / 4.8 s (the input of 7.9), two overlapping sources in sensor
noise, K = 3 classes.

  the aligner               pk2_perm_align on the masks of the blind EM, buffers allocated beforehand, with and without the
                            covariances; its stages by differences: refine = 1 against refine = 3
  the torch formulation     the same mathematics in torch ops (float64 sums through einsum, the tree level by level, the
                            K! candidates as one gather), per utterance on the same device, alternating with ours run by run
  around it                 the blind EM (cgmm_masks, init='random', 20 iterations), CgmmSeparator.masks (EM + aligner),
                            separate (covariances, MVDR weights and apply for the eight (utterance, speaker) pairs)

each the median (min, max) of 10 runs between device events after 2 warm-up runs.

    python tools/sep_time.py [--out FILE]
"""
import argparse
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beamform_time import CHANNELS, SECONDS, device_times  # noqa: E402

K, ITERS, REFINE = 3, 20, 3


def lines():
    import torch
    from pykaldi2_amd import _lib, beamform, cgmm, separate, simulation
    dev = torch.device("cuda")
    an = simulation.SpectrumAnalyzer(do_dither=False)
    bf = beamform.MaskBeamformer(an)
    gen = torch.Generator(device="cuda").manual_seed(0)
    wavs = []
    for s in SECONDS:      # two sources with on/off stretches of half a second, delays of c and 2 - c samples at microphone c
        n = int(round(16000 * s))
        mix = 0.0224 * torch.randn(CHANNELS, n, device=dev, generator=gen)
        for j in range(2):
            on = (torch.rand((n + 7999) // 8000, device=dev, generator=gen) < 0.6).repeat_interleave(8000)[:n]
            src = 0.1 * torch.randn(n, device=dev, generator=gen) * on
            mix = mix + torch.stack([torch.roll(src, c if j == 0 else 2 - c) for c in range(CHANNELS)])
        wavs.append(mix)
    specs = [bf.analyze(x) for x in wavs]
    frames = [int(s.shape[1]) for s in specs]
    B, F, Cn = len(specs), an.n_bin, CHANNELS
    L, stream = _lib.lib(), _lib.stream_ptr(dev)
    masks = cgmm.cgmm_masks(specs, K, ITERS, init="random", seed=0)
    R = torch.stack(cgmm.last_cov).contiguous()
    la = torch.stack(cgmm.last_log_alpha).contiguous()

    def table(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    fr = (C.c_int32 * B)(*frames)
    nbytes = L.pk2_perm_align_workspace_bytes(fr, B, F, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = [torch.empty_like(m) for m in masks]
    Ro, lao = torch.empty_like(R), torch.empty_like(la)
    perm = torch.empty(B, F, K, dtype=torch.int32, device=dev)
    margin = torch.empty(B, F, dtype=torch.float32, device=dev)
    t_masks, t_out = table(masks), table(out)

    def align(refine=REFINE, with_cov=True):
        _lib.check(L.pk2_perm_align(t_masks, _lib.ptr(R) if with_cov else None, _lib.ptr(la) if with_cov else None, fr, B,
                                    Cn if with_cov else 0, F, K, refine, 1, _lib.ptr(work), nbytes, t_out,
                                    _lib.ptr(Ro) if with_cov else None, _lib.ptr(lao) if with_cov else None, _lib.ptr(perm),
                                    _lib.ptr(margin), stream))

    P = torch.tensor(list(itertools.permutations(range(K))), device=dev)                  # (K!, K)
    ar = torch.arange(K, device=dev)

    def pearson(v):
        d = v - v.mean(-1, keepdim=True)
        return d / d.norm(dim=-1, keepdim=True).clamp_min(1e-10)

    def best(S):
        return P[S[..., ar, P].sum(-1).argmax(-1)]                                         # (..., K)

    t_perm = [None] * B

    def torch_align():
        for b in range(B):
            u = pearson(masks[b].double().permute(2, 0, 1)).float()                        # (F, K, N)
            pi = ar.expand(F, K).contiguous()
            cent, weight, level, bins = u.double(), torch.ones(F, dtype=torch.float64, device=dev), 0, torch.arange(F, device=dev)
            while cent.shape[0] > 1:
                m = cent.shape[0] // 2
                cl, cr = cent[0:2 * m:2], cent[1:2 * m:2]
                p = best(torch.einsum("gan,gbn->gab", cl, cr))                             # (m, K)
                g = bins >> level
                right = ((g & 1) == 1) & ((g >> 1) < m)
                pi = torch.where(right[:, None], torch.gather(pi, 1, p[(g >> 1).clamp_max(m - 1)]), pi)
                wl, wr = weight[0:2 * m:2], weight[1:2 * m:2]
                merged = pearson(wl[:, None, None] * cl + wr[:, None, None] * torch.gather(cr, 1, p[:, :, None].expand_as(cr)))
                merged, nw = merged.float().double(), wl + wr
                if cent.shape[0] % 2:
                    merged, nw = torch.cat([merged, cent[-1:]]), torch.cat([nw, weight[-1:]])
                cent, weight, level = merged, nw, level + 1
            ud = u.double()
            for _ in range(REFINE):
                up = torch.gather(ud, 1, pi[:, :, None].expand_as(ud))
                c = pearson(up.sum(0)).float().double()
                pi = torch.gather(pi, 1, best(torch.einsum("an,fbn->fab", c, up)))
            pur = (R[b].abs() ** 2).sum((-2, -1)).double() / torch.diagonal(R[b], dim1=-2, dim2=-1).real.sum(-1).double() ** 2
            q = torch.gather(pur, 0, pi.t()).sum(1)
            order = torch.sort((ar == q.argmin()).int(), stable=True).indices               # the noise stream last
            pi = pi[:, order]
            t_perm[b] = pi
            out[b].copy_(torch.gather(masks[b], 0, pi.t()[:, None, :].expand_as(masks[b])))

    align()
    ours = perm.clone()
    torch_align()
    torch.cuda.synchronize()
    same = [float((t_perm[b] == ours[b]).all(1).float().mean()) for b in range(B)]
    res = ["C %d, K %d, fft 512 / 400 / 160, utterances of %s s = frames %s, masks %.1f MB; workspace %.1f MB; blind EM of %d "
           "iterations from init='random', seed 0" % (Cn, K, "/".join(str(s) for s in SECONDS), frames,
                                                      sum(m.numel() for m in masks) * 4 / 1e6, nbytes / 1e6, ITERS),
           "bins on which ours and the torch formulation choose the same order, per utterance: %s; smallest margin %.3f, "
           "median %.3f" % (" ".join("%.3f" % x for x in same), float(margin.min()), float(margin.median()))]
    a, t = device_times([align, torch_align])
    res += ["aligner with covariances, %d rounds, pk2_perm_align: %s" % (REFINE, a), "aligner, the torch formulation: %s" % t]
    res += ["aligner with 1 round: %s" % device_times([lambda: align(1)])[0]]
    res += ["aligner with 8 rounds: %s" % device_times([lambda: align(8)])[0]]
    res += ["aligner without covariances, %d rounds: %s" % (REFINE, device_times([lambda: align(REFINE, False)])[0])]
    res += ["separate.align_permutations (pk2_perm_align and its allocations): %s"
            % device_times([lambda: separate.align_permutations(masks, list(R.unbind(0)), list(la.unbind(0)))])[0]]
    res += ["blind EM, cgmm.cgmm_masks(K = %d, %d iterations, init='random'; host draws and upload included): %s"
            % (K, ITERS, device_times([lambda: cgmm.cgmm_masks(specs, K, ITERS, init="random", seed=0)])[0])]
    init = [_lib.h2d(cgmm.random_init(K, n, F, 0, i), dev) for i, n in enumerate(frames)]
    res += ["blind EM from masks already on the device: %s"
            % device_times([lambda: cgmm.cgmm_masks(specs, K, ITERS, init=init)])[0]]
    sep = separate.CgmmSeparator(an, K - 1, ITERS)
    res += ["CgmmSeparator.masks (EM + aligner): %s" % device_times([lambda: sep.masks(specs)])[0]]
    aligned = sep.masks(specs)
    res += ["separate (covariances, MVDR weights, apply for %d (utterance, speaker) pairs): %s"
            % (B * (K - 1), device_times([lambda: separate.separate(specs, aligned)])[0])]
    res += ["clone() of the four mask sets (the floor of one pass): %s" % device_times([lambda: [m.clone() for m in masks]])[0]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sep_time.txt"))
    args = ap.parse_args()
    res = lines()
    with open(args.out, "w") as f:
        f.write("\n".join(res) + "\n")
    print("\n".join(res))


if __name__ == "__main__":
    main()
