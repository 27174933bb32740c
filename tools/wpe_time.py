"""Device time of WPE dereverberation, written to profiles/wpe_time.txt: C = 7 channels, fft 512 / frame 400
/ shift 160, four utterances of 4.4 / 16.2 / 17.1 / 4.8 s (the durations of the LF-MMI benchmark's first minibatch), 10 taps,
delay 3, 3 iterations.

  each stage alone          pk2_wpe_power, pk2_wpe_corr, pk2_wpe_solve, pk2_wpe_filter: one call each for the minibatch, buffers
                            allocated beforehand
  the whole                 pk2_wpe (3 iterations, nothing read back) and dereverb.wpe (the same with its allocations)
  the torch formulation     the same stages per utterance on the same device in the same run, alternating with ours run by run:
                            the stacked (F, N, D) matrix by shifted views, batched complex64 matmul, linalg.solve in complex128
  the floor of one pass     clone() of the four spectra

each the median (min, max) of 10 runs between device events after 2 warm-up runs.

Expected before the first run: the correlation stage is the arithmetic, 6 tile pairs x 4 x 32 x 32 real FMAs per frame and
bin = 26.8 G real FMAs per iteration, 0.34 ms at the 157 TFLOP/s matrix peak; with one LDS read pair per four MFMAs and no
software pipelining a third to two thirds of the peak, 0.5 to 1 ms.  The filter is 2.4 G FMAs on the vector units behind LDS
reads of G, 0.1 to 0.2 ms; the solve 1028 workgroups of a few thousand barriers, 0.1 to 0.3 ms.  The whole: 3 ms or less.
The torch formulation: several times that, its stacked matrix is 10 x the spectrum, written and read twice per iteration.

    python tools/wpe_time.py [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDS = (4.4, 16.2, 17.1, 4.8)
CHANNELS, TAPS, DELAY, ITERS, DIAG_LOAD = 7, 10, 3, 3, 1e-3


def device_times(fns, runs=10, warmup=2):
    """the callables run alternately, one after the other in every round; returns (summary strings, medians in ms)"""
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
    return (["median %.4f ms (min %.4f, max %.4f) of %d" % (float(np.median(t)), min(t), max(t), runs) for t in times],
            [float(np.median(t)) for t in times])


def lines():
    import torch
    from pykaldi2_amd import _lib, dereverb, simulation
    dev = torch.device("cuda")
    an = simulation.SpectrumAnalyzer(do_dither=False)
    drv = dereverb.Dereverberator(an, TAPS, DELAY, ITERS, DIAG_LOAD)
    gen = torch.Generator(device="cuda").manual_seed(0)
    # reverberant-looking input: white noise through a decaying random FIR per channel, so that the solves are those of a
    # coherent source and not of an identity matrix
    wavs = []
    for s in SECONDS:
        n = int(round(16000 * s))
        src = torch.randn(1, 1, n + 3999, device=dev, generator=gen)
        fir = torch.randn(CHANNELS, 1, 4000, device=dev, generator=gen) * torch.exp(-torch.arange(4000, device=dev) / 800.0).flip(0)
        wavs.append((0.02 * torch.nn.functional.conv1d(src, fir)[0] + 1e-3 * torch.randn(CHANNELS, n, device=dev, generator=gen))
                    .contiguous())
    specs = [drv.analyze(x) for x in wavs]
    frames = [int(s.shape[1]) for s in specs]
    B, F, D = len(specs), an.n_bin, CHANNELS * TAPS
    spec_mb = sum(s.numel() for s in specs) * 8 / 1e6
    L, stream = _lib.lib(), _lib.stream_ptr(dev)

    def table(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    fr = (C.c_int32 * B)(*frames)
    nbytes = L.pk2_wpe_workspace_bytes(fr, B, CHANNELS, F, TAPS, DELAY)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pw = [torch.empty(n, F, dtype=torch.float32, device=dev) for n in frames]
    pw2 = [torch.empty(n, F, dtype=torch.float32, device=dev) for n in frames]
    Rm = torch.empty(B, F, D, D, dtype=torch.complex64, device=dev)
    Pm = torch.empty(B, F, D, CHANNELS, dtype=torch.complex64, device=dev)
    G = torch.empty(B, F, D, CHANNELS, dtype=torch.complex64, device=dev)
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    outs = [torch.empty_like(s) for s in specs]
    t_spec, t_pw, t_pw2, t_out = table(specs), table(pw), table(pw2), table(outs)

    def power():
        _lib.check(L.pk2_wpe_power(t_spec, fr, B, CHANNELS, F, t_pw, stream))

    def corr():
        _lib.check(L.pk2_wpe_corr(t_spec, t_pw, fr, B, CHANNELS, F, TAPS, DELAY, _lib.ptr(work), nbytes, _lib.ptr(Rm), _lib.ptr(Pm),
                                  stream))

    def solve():
        _lib.check(L.pk2_wpe_solve(_lib.ptr(Rm), _lib.ptr(Pm), B, CHANNELS, F, TAPS, DIAG_LOAD, _lib.ptr(work), nbytes, _lib.ptr(G),
                                   _lib.ptr(flag), stream))

    def filt():
        _lib.check(L.pk2_wpe_filter(t_spec, _lib.ptr(G), fr, B, CHANNELS, F, TAPS, DELAY, t_out, t_pw2, stream))

    def whole():
        _lib.check(L.pk2_wpe(t_spec, fr, B, CHANNELS, F, TAPS, DELAY, ITERS, DIAG_LOAD, _lib.ptr(work), nbytes, t_out,
                             _lib.ptr(flag), stream))

    # the same stages in torch, per utterance; bin-major copies of the spectra are made beforehand (not timed)
    Yf = [s.permute(2, 1, 0).contiguous() for s in specs]                      # (F, N, C)
    t_lam = [None] * B
    t_R, t_P, t_G, t_X = [None] * B, [None] * B, [None] * B, [None] * B
    eye = torch.eye(D, dtype=torch.complex128, device=dev)

    def stacked(y):
        N = y.shape[1]
        Z = torch.zeros(F, N, D, dtype=torch.complex64, device=dev)
        for k in range(TAPS):
            s = DELAY + k
            Z[:, s:, k * CHANNELS:(k + 1) * CHANNELS] = y[:, :N - s]             # shifted views of the spectrum
        return Z

    def torch_power(src=None):
        for b in range(B):
            x = Yf[b] if src is None else src[b]
            t_lam[b] = (x.real ** 2 + x.imag ** 2).mean(-1).clamp_min(1e-10)      # (F, N)

    def torch_corr():
        for b in range(B):
            Z = stacked(Yf[b])
            Zw = (Z / t_lam[b][:, :, None]).transpose(1, 2)                       # (F, D, N)
            t_R[b] = torch.matmul(Zw, Z.conj())
            t_P[b] = torch.matmul(Zw, Yf[b].conj())

    def torch_solve():
        for b in range(B):
            Rd = t_R[b].to(torch.complex128)
            load = DIAG_LOAD * torch.diagonal(Rd, dim1=-2, dim2=-1).real.sum(-1) / D + 1e-10
            t_G[b] = torch.linalg.solve(Rd + load[:, None, None] * eye, t_P[b].to(torch.complex128)).to(torch.complex64)

    def torch_filter():
        for b in range(B):
            t_X[b] = Yf[b] - torch.matmul(stacked(Yf[b]), t_G[b].conj())

    def torch_whole():
        torch_power()
        for it in range(ITERS):
            torch_corr()
            torch_solve()
            torch_filter()
            torch_power(t_X)
        return [x.permute(2, 1, 0).contiguous() for x in t_X]

    power()
    corr()
    solve()
    filt()
    torch_power()
    torch_corr()
    torch_solve()
    torch_filter()
    torch.cuda.synchronize()
    err_R = max(float((t_R[b] - Rm[b]).abs().max() / Rm[b].abs().max()) for b in range(B))
    err_P = max(float((t_P[b] - Pm[b]).abs().max() / Pm[b].abs().max()) for b in range(B))
    err_G = max(float((t_G[b] - G[b]).abs().max() / G[b].abs().max()) for b in range(B))
    err_X = max(float((t_X[b].permute(2, 1, 0) - outs[b]).abs().max() / outs[b].abs().max()) for b in range(B))
    whole()
    tw = torch_whole()
    torch.cuda.synchronize()
    err_W = max(float((tw[b] - outs[b]).abs().max() / outs[b].abs().max()) for b in range(B))
    total = sum(frames)
    E = D + CHANNELS
    tiles = (E + 31) // 32
    fma_exec = total * F * (tiles * (tiles + 1) // 2) * 4 * 1024                 # real FMAs the MFMAs execute
    fma_need = total * F * 4 * (D * (D + 1) // 2 + D * CHANNELS)                  # of the lower triangle of R and of P
    res = ["C %d, taps %d, delay %d, %d iterations, fft 512 / 400 / 160, utterances of %s s = frames %s, spectra %.1f MB; "
           "workspace %.1f MB" % (CHANNELS, TAPS, DELAY, ITERS, "/".join(str(s) for s in SECONDS), frames, spec_mb, nbytes / 1e6),
           "ours against the torch formulation, one iteration: R rel diff %.2e, P %.2e, G %.2e, X %.2e; three iterations: X %.2e"
           % (err_R, err_P, err_G, err_X, err_W), "non-finite flags of the whole: %s" % flag.tolist()]
    (ours, theirs), _ = device_times([power, torch_power])
    res += ["power, pk2_wpe_power: %s" % ours, "power, torch: %s" % theirs]
    (ours, theirs), (ms, _) = device_times([corr, torch_corr])
    res += ["correlations, pk2_wpe_corr (both transposing pre-passes, MFMA pass, reduction): %s" % ours,
            "correlations, torch (stacked matrix by shifted views, complex64 matmul): %s" % theirs,
            "correlations: %.2f G real FMAs executed by the MFMAs (%.2f G of them in the lower triangle of R and in P) = %.1f "
            "TFLOP/s executed, %.1f %% of the 157 TFLOP/s matrix peak (%.1f %% counting the needed ones only)"
            % (fma_exec / 1e9, fma_need / 1e9, 2 * fma_exec / ms / 1e9, 100 * 2 * fma_exec / ms / 1e9 / 157.3,
               100 * 2 * fma_need / ms / 1e9 / 157.3)]
    (ours, theirs), _ = device_times([solve, torch_solve])
    res += ["solve, pk2_wpe_solve: %s" % ours, "solve, torch.linalg.solve in complex128: %s" % theirs]
    (ours, theirs), _ = device_times([filt, torch_filter])
    res += ["filter with the next power, pk2_wpe_filter: %s" % ours, "filter, torch (stacked matrix, complex64 matmul): %s" % theirs]
    (ours, theirs), (ms, _) = device_times([whole, torch_whole])
    res += ["the whole, pk2_wpe: %s" % ours, "the whole, torch: %s" % theirs,
            "the whole per utterance of the minibatch: %.3f ms" % (ms / B)]
    res += ["dereverb.wpe (pk2_wpe with its allocations): %s" % device_times([lambda: dereverb.wpe(specs, TAPS, DELAY, ITERS, DIAG_LOAD)])[0][0]]
    res += ["clone() of the four spectra (the floor of one pass): %s" % device_times([lambda: [s.clone() for s in specs]])[0][0]]
    res += ["Dereverberator.batch (STFT, pk2_wpe, inverse STFT): %s" % device_times([lambda: drv.batch(wavs)])[0][0]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpe_time.txt"))
    args = ap.parse_args()
    res = lines()
    with open(args.out, "w") as f:
        f.write("\n".join(res) + "\n")
    print("\n".join(res))


if __name__ == "__main__":
    main()
