"""Device time of the cGMM mask estimator, written to profiles/cgmm_time.txt: C = 7 channels, fft 512 /
frame 400 / shift 160, four utterances of 4.4 / 16.2 / 17.1 / 4.8 s (the durations of the LF-MMI benchmark's first
minibatch), K = 2 classes, 10 iterations.

  each stage alone          pk2_cgmm_factor, pk2_cgmm_posteriors, pk2_cgmm_update: one call each for the minibatch, buffers
                            allocated beforehand
  the whole EM              pk2_cgmm (start state, 10 iterations, class order), and cgmm.cgmm_masks with its allocations
  the torch formulation     the same stages with torch.einsum for the quadratic forms and the weighted covariances and
                            torch.linalg.cholesky in complex128, per utterance on the same device in the same run,
                            alternating with ours run by run
  the floor of one pass     clone() of the four spectra

each the median (min, max) of 10 runs between device events after 2 warm-up runs.

    python tools/cgmm_time.py [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beamform_time import CHANNELS, SECONDS, device_times  # noqa: E402

K, ITERS, DIAG_LOAD = 2, 10, 1e-3


def lines():
    import torch
    from pykaldi2_amd import _lib, beamform, cgmm, simulation
    dev = torch.device("cuda")
    an = simulation.SpectrumAnalyzer(do_dither=False)
    bf = beamform.MaskBeamformer(an)
    gen = torch.Generator(device="cuda").manual_seed(0)
    wavs = []
    for s in SECONDS:      # a source that reaches microphone c with a delay of c samples, in sensor noise 10 dB below it
        n = int(round(16000 * s))
        src = 0.1 * torch.randn(n, device=dev, generator=gen) * (torch.rand(n, device=dev, generator=gen) < 0.5)
        wavs.append(torch.stack([torch.roll(src, c) for c in range(CHANNELS)])
                    + 0.0224 * torch.randn(CHANNELS, n, device=dev, generator=gen))
    specs = [bf.analyze(x) for x in wavs]
    frames = [int(s.shape[1]) for s in specs]
    B, F, Cn = len(specs), an.n_bin, CHANNELS
    spec_mb = sum(s.numel() for s in specs) * 8 / 1e6
    L, stream = _lib.lib(), _lib.stream_ptr(dev)

    def table(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    fr = (C.c_int32 * B)(*frames)
    nbytes = L.pk2_cgmm_workspace_bytes(fr, B, Cn, F, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    R = torch.empty(B, K, F, Cn, Cn, dtype=torch.complex64, device=dev)
    la = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    R1, la1 = torch.empty_like(R), torch.empty_like(la)
    linv = torch.empty(B, K, Cn * (Cn + 1), F, dtype=torch.float32, device=dev)
    bias = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    bad = torch.empty(B, K, F, dtype=torch.int32, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    lam = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    phi = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    masks = [torch.empty(K, n, F, dtype=torch.float32, device=dev) for n in frames]
    ll1 = torch.empty(B, dtype=torch.float64, device=dev)
    ll = torch.empty(B, ITERS, dtype=torch.float64, device=dev)
    t_spec, t_lam, t_phi, t_masks = table(specs), table(lam), table(phi), table(masks)

    def init():
        _lib.check(L.pk2_cgmm_init(t_spec, None, None, fr, B, Cn, F, K, _lib.ptr(work), nbytes, _lib.ptr(R), _lib.ptr(la), stream))

    def factor():
        _lib.check(L.pk2_cgmm_factor(_lib.ptr(R), _lib.ptr(la), B, Cn, F, K, DIAG_LOAD, _lib.ptr(linv), _lib.ptr(bias),
                                     _lib.ptr(bad), _lib.ptr(flag), stream))

    def posteriors():
        _lib.check(L.pk2_cgmm_posteriors(t_spec, None, fr, B, Cn, F, K, _lib.ptr(linv), _lib.ptr(bias), _lib.ptr(bad),
                                         _lib.ptr(work), nbytes, t_lam, t_phi, _lib.ptr(ll1), stream))

    def update():
        _lib.check(L.pk2_cgmm_update(t_spec, t_lam, t_phi, None, fr, B, Cn, F, K, _lib.ptr(work), nbytes, _lib.ptr(R1),
                                     _lib.ptr(la1), stream))

    def whole():
        _lib.check(L.pk2_cgmm(t_spec, None, None, fr, B, Cn, F, K, ITERS, DIAG_LOAD, 1, _lib.ptr(work), nbytes, t_masks,
                              _lib.ptr(R1), _lib.ptr(la1), _lib.ptr(ll), _lib.ptr(flag), stream))

    # the same stages in torch, per utterance; the identity is made beforehand
    eye = torch.eye(Cn, dtype=torch.complex128, device=dev)
    t_state = [None] * B      # (R complex64 (K, F, C, C), log alpha (K, F))
    t_fac = [None] * B        # (L^-1 complex64 (K, F, C, C), b (K, F))
    t_post = [None] * B       # (lam (K, N, F), phi (K, N, F), ll)

    def torch_init():
        for b in range(B):
            R0 = torch.einsum("ctf,dtf->fcd", specs[b], specs[b].conj()) / frames[b]
            tr = torch.diagonal(R0, dim1=-2, dim2=-1).real.sum(-1) / Cn
            t_state[b] = (torch.stack([R0, tr[:, None, None] * eye.to(torch.complex64)]),
                          torch.full((K, F), -0.6931472, device=dev))

    def torch_factor():
        for b in range(B):
            Rb, lab = t_state[b]
            Rd = Rb.to(torch.complex128)
            load = DIAG_LOAD * torch.diagonal(Rd, dim1=-2, dim2=-1).real.sum(-1) / Cn + 1e-10
            Lc = torch.linalg.cholesky(Rd + load[..., None, None] * eye)
            Li = torch.linalg.solve_triangular(Lc, eye.expand_as(Lc), upper=False)
            bb = lab.double() - 2 * torch.log(torch.diagonal(Lc, dim1=-2, dim2=-1).real).sum(-1)
            t_fac[b] = (Li.to(torch.complex64), bb.float())

    def torch_posteriors():
        for b in range(B):
            Li, bb = t_fac[b]
            z = torch.einsum("kfij,jtf->ktfi", Li, specs[b])
            ph = ((z.real ** 2 + z.imag ** 2).sum(-1) / Cn).clamp_min(1e-10)
            ell = bb[:, None, :] - Cn * torch.log(ph)
            lse = torch.logsumexp(ell, dim=0)
            t_post[b] = (torch.exp(ell - lse[None]), ph, lse.double().sum())

    def torch_update():
        for b in range(B):
            lm, ph, _ = t_post[b]
            yy = torch.einsum("ctf,dtf->tfcd", specs[b], specs[b].conj())                  # (N, F, C, C)
            sm = lm.sum(1)
            Rn = torch.einsum("ktf,tfcd->kfcd", (lm / ph).to(torch.complex64), yy) / sm.clamp_min(1e-10)[:, :, None, None]
            t_state[b] = (Rn, torch.log((sm / frames[b]).clamp_min(1e-10)))

    def torch_whole():
        torch_init()
        for _ in range(ITERS):
            torch_factor()
            torch_posteriors()
            torch_update()

    # agreement: one iteration of ours on the torch state, then the whole EM (in the order 'keep' both)
    init()
    torch_init()
    torch.cuda.synchronize()
    err_init = max(float((t_state[b][0] - R[b]).abs().max() / R[b].abs().max()) for b in range(B))
    factor()
    posteriors()
    update()
    torch_factor()
    torch_posteriors()
    torch_update()
    torch.cuda.synchronize()
    err_lam = max(float((t_post[b][0] - lam[b]).abs().max()) for b in range(B))
    err_R = max(float((t_state[b][0] - R1[b]).abs().max() / R1[b].abs().max()) for b in range(B))
    res = ["C %d, K %d, %d iterations, fft 512 / 400 / 160, utterances of %s s = frames %s, spectra %.1f MB, masks %.1f MB; "
           "workspace %.1f MB" % (Cn, K, ITERS, "/".join(str(s) for s in SECONDS), frames, spec_mb,
                                  sum(m.numel() for m in masks) * 4 / 1e6, nbytes / 1e6),
           "ours against the torch formulation after one iteration: start state rel diff %.2e, posteriors abs diff %.2e, "
           "covariance rel diff %.2e" % (err_init, err_lam, err_R)]
    # the stage timings run on the state after the first iteration (torch_update changed t_state, so put the start back)
    torch_init()
    ours, theirs = device_times([factor, torch_factor])
    res += ["factor, pk2_cgmm_factor: %s" % ours, "factor, torch.linalg.cholesky + solve_triangular in complex128: %s" % theirs]
    ours, theirs = device_times([posteriors, torch_posteriors])
    res += ["posteriors, pk2_cgmm_posteriors: %s" % ours, "posteriors, torch.einsum + logsumexp: %s" % theirs]
    ours, theirs = device_times([update, torch_update])
    res += ["update, pk2_cgmm_update: %s" % ours, "update, torch.einsum: %s" % theirs]
    ours, theirs = device_times([whole, torch_whole])
    res += ["whole EM (start state, %d iterations, class order), pk2_cgmm: %s" % (ITERS, ours),
            "whole EM, the torch formulation: %s" % theirs]
    res += ["cgmm.cgmm_masks (pk2_cgmm and its allocations): %s" % device_times([lambda: cgmm.cgmm_masks(specs, K, ITERS)])[0]]
    res += ["start state alone, pk2_cgmm_init: %s" % device_times([init])[0]]
    res += ["clone() of the four spectra (the floor of one pass): %s" % device_times([lambda: [s.clone() for s in specs]])[0]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cgmm_time.txt"))
    args = ap.parse_args()
    res = lines()
    with open(args.out, "w") as f:
        f.write("\n".join(res) + "\n")
    print("\n".join(res))


if __name__ == "__main__":
    main()
