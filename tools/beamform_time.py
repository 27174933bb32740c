"""Device time of the mask-based MVDR beamformer, written to profiles/beamform_time.txt: C = 7 channels,
fft 512 / frame 400 / shift 160, and four utterances of 4.4 / 16.2 / 17.1 / 4.8 s (the durations of the LF-MMI benchmark's
first minibatch), speech mask plus complement.

  each stage alone          pk2_bf_cov, pk2_bf_mvdr_weights (ref 0 and 'snr'), pk2_bf_apply: one launch each for the minibatch,
                            buffers allocated beforehand
  MaskBeamformer.batch      as the data pipeline calls it: 4 STFT launches, the three stages, 4 inverse STFTs, allocations
  the torch formulation     the same three stages with torch.einsum / torch.linalg.solve per utterance on the same device in
                            the same run, alternating with ours run by run
  the floor of one pass     clone() of the four spectra

each the median (min, max) of 10 runs between device events after 2 warm-up runs.

    python tools/beamform_time.py [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDS = (4.4, 16.2, 17.1, 4.8)
CHANNELS = 7


def device_times(fns, runs=10, warmup=2):
    """the callables run alternately, one after the other in every round; returns one summary string per callable"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return ["median %.4f ms (min %.4f, max %.4f) of %d" % (float(np.median(t)), min(t), max(t), runs) for t in times]


def lines():
    import torch
    from pykaldi2_amd import _lib, beamform, simulation
    dev = torch.device("cuda")
    an = simulation.SpectrumAnalyzer(do_dither=False)
    bf = beamform.MaskBeamformer(an)
    gen = torch.Generator(device="cuda").manual_seed(0)
    wavs = [0.1 * torch.randn(CHANNELS, int(round(16000 * s)), device=dev, generator=gen) for s in SECONDS]
    specs = [bf.analyze(x) for x in wavs]
    masks = [torch.rand(s.shape[1], s.shape[2], device=dev, generator=gen) for s in specs]
    frames = [int(s.shape[1]) for s in specs]
    B, F = len(specs), an.n_bin
    spec_mb = sum(s.numel() for s in specs) * 8 / 1e6
    L, stream = _lib.lib(), _lib.stream_ptr(dev)

    def table(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    fr = (C.c_int32 * B)(*frames)
    nbytes = L.pk2_bf_workspace_bytes(fr, B, CHANNELS, F, 1, 1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    phi = torch.empty(B, 2, F, CHANNELS, CHANNELS, dtype=torch.complex64, device=dev)
    w = torch.empty(B, F, CHANNELS, dtype=torch.complex64, device=dev)
    idx, flag = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    outs = [torch.empty(n, F, dtype=torch.complex64, device=dev) for n in frames]
    t_spec, t_mask, t_out = table(specs), table(masks), table(outs)
    t_ps, t_pn, t_w = table([phi[b, 0] for b in range(B)]), table([phi[b, 1] for b in range(B)]), table([w[b] for b in range(B)])

    def cov():
        _lib.check(L.pk2_bf_cov(t_spec, t_mask, fr, B, CHANNELS, F, 1, 1, _lib.ptr(work), nbytes, _lib.ptr(phi), stream))

    def weights(ref):
        _lib.check(L.pk2_bf_mvdr_weights(t_ps, t_pn, B, CHANNELS, F, ref, 1e-3, _lib.ptr(work), nbytes, _lib.ptr(w), _lib.ptr(idx),
                                         _lib.ptr(flag), stream))

    def apply():
        _lib.check(L.pk2_bf_apply(t_spec, t_w, fr, B, CHANNELS, F, t_out, stream))

    # the same stages in torch; the masks as complex tensors and the identity are made beforehand
    cmasks = [torch.stack([m, 1 - m]).to(torch.complex64) for m in masks]
    msums = [torch.stack([m.sum(0), (1 - m).sum(0)]).clamp_min(1e-10) for m in masks]
    eye = torch.eye(CHANNELS, dtype=torch.complex128, device=dev)
    t_phi, t_wts = [None] * B, [None] * B

    def torch_cov():
        for b in range(B):
            yy = torch.einsum("ctf,dtf->tfcd", specs[b], specs[b].conj())                  # (N, F, C, C)
            t_phi[b] = torch.einsum("ktf,tfcd->kfcd", cmasks[b], yy) / msums[b][:, :, None, None]

    def torch_weights():
        for b in range(B):
            ps, pn = t_phi[b][0].to(torch.complex128), t_phi[b][1].to(torch.complex128)
            load = 1e-3 * torch.diagonal(pn, dim1=-2, dim2=-1).real.sum(-1) / CHANNELS + 1e-10
            G = torch.linalg.solve(pn + load[:, None, None] * eye, ps)
            t_wts[b] = (G[:, :, 0] / torch.diagonal(G, dim1=-2, dim2=-1).sum(-1, keepdim=True)).to(torch.complex64)

    def torch_apply():
        return [torch.einsum("fc,ctf->tf", t_wts[b].conj(), specs[b]) for b in range(B)]

    cov()
    weights(0)
    torch_cov()
    torch_weights()
    torch.cuda.synchronize()
    err_phi = max(float((t_phi[b] - phi[b]).abs().max() / phi[b].abs().max()) for b in range(B))
    err_w = max(float((t_wts[b] - w[b]).abs().max() / w[b].abs().max()) for b in range(B))
    res = ["C %d, fft 512 / 400 / 160, utterances of %s s = frames %s, spectra %.1f MB, masks %.1f MB; workspace %.1f MB"
           % (CHANNELS, "/".join(str(s) for s in SECONDS), frames, spec_mb, sum(m.numel() for m in masks) * 4 / 1e6, nbytes / 1e6),
           "ours against the torch formulation: covariance rel diff %.2e, weights rel diff %.2e" % (err_phi, err_w)]
    ours, theirs = device_times([cov, torch_cov])
    res += ["covariance (mask + complement), pk2_bf_cov: %s" % ours, "covariance, torch.einsum: %s" % theirs]
    ours, theirs = device_times([lambda: weights(0), torch_weights])
    res += ["weights ref 0, pk2_bf_mvdr_weights: %s" % ours, "weights ref 0, torch.linalg.solve in complex128: %s" % theirs]
    res += ["weights ref 'snr', pk2_bf_mvdr_weights: %s" % device_times([lambda: weights(_lib.BF_REF_SNR)])[0]]
    weights(0)
    ours, theirs = device_times([apply, torch_apply])
    res += ["apply, pk2_bf_apply: %s" % ours, "apply, torch.einsum: %s" % theirs]
    res += ["clone() of the four spectra (the floor of one pass): %s" % device_times([lambda: [s.clone() for s in specs]])[0]]
    res += ["MaskBeamformer.batch (STFT, three stages, inverse STFT): %s" % device_times([lambda: bf.batch(wavs, masks)])[0]]
    res += ["STFT of the four utterances alone: %s" % device_times([lambda: [bf.analyze(x) for x in wavs]])[0]]
    res += ["inverse STFT of the four outputs alone: %s" % device_times([lambda: [an.synthesize(o) for o in outs]])[0]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beamform_time.txt"))
    args = ap.parse_args()
    res = lines()
    with open(args.out, "w") as f:
        f.write("\n".join(res) + "\n")
    print("\n".join(res))


if __name__ == "__main__":
    main()
