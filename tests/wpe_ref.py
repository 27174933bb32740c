"""A numpy restatement of WPE dereverberation as DESIGN.md 7.10 fixes it, in float64, with a float32 mode that rounds where
the kernels round (complex64 correlation sums in frame order, a float64 solve, a complex64 G, a complex64 filter): the yardstick
of tests/test_wpe_host.py and tests/test_gpu_wpe.py.  Not part of the package.

Spectra are (C, N, F); y~(t)[k C + c] = Y[c, t - delay - k, f], zero before the first frame; D = C taps."""
import numpy as np

FLOOR = 1e-10
P = 1024          # frames per float32 chain of the device's correlation pass (PK2_WPE_FRAMES_PER_PART)


def stack_past(Y, taps, delay):
    """(C, N, F) -> (F, N, D)"""
    Cn, N, F = Y.shape
    out = np.zeros((F, N, taps * Cn), Y.dtype)
    for k in range(taps):
        s = delay + k
        if s < N:
            out[:, s:, k * Cn:(k + 1) * Cn] = Y[:, :N - s, :].transpose(2, 1, 0)
    return out


def power(X, dtype=np.float64):
    """(C, N, F) -> (N, F): max(sum_c |X|^2 / C, 1e-10); the sum in channel order"""
    X = np.asarray(X)
    s = np.zeros(X.shape[1:], dtype)
    for c in range(X.shape[0]):
        s = s + X[c].real.astype(dtype) ** 2
        s = s + X[c].imag.astype(dtype) ** 2
    return np.maximum(s / dtype(X.shape[0]), dtype(FLOOR))


def correlations(Y, weight, taps, delay, dtype=np.float64):
    """R (F, D, D) = sum_t y~ y~^H / weight, P (F, D, C) = sum_t y~ Y^H / weight.  float32: the rows times the float32
    reciprocal of the weight, complex64 sums in frame order."""
    ct = np.complex64 if dtype == np.float32 else np.complex128
    Y = np.asarray(Y).astype(ct)
    Cn, N, F = Y.shape
    D = Cn * taps
    Z = np.concatenate([stack_past(Y, taps, delay), Y.transpose(2, 1, 0)], axis=2)        # (F, N, D + C)
    inv = (dtype(1) / np.asarray(weight).astype(dtype)).T                                  # (F, N)
    if dtype == np.float32:
        acc = np.zeros((F, D, D + Cn), ct)
        for t in range(N):
            zw = Z[:, t, :D] * inv[:, t, None]
            acc += zw[:, :, None] * Z[:, t, None, :].conj()
    else:
        acc = np.einsum("ftd,fte->fde", Z[:, :, :D] * inv[:, :, None], Z.conj())
    R, Pm = acc[:, :, :D].copy(), acc[:, :, D:].copy()
    # exactly Hermitian with a real diagonal, from the lower triangle (as the device writes it)
    low = np.tril(R, -1)
    R = low + low.conj().transpose(0, 2, 1) + np.einsum("fdd->fd", R).real[:, :, None] * np.eye(D)
    return R.astype(ct), Pm


def load(R, diag_load):
    D = R.shape[-1]
    tr = np.einsum("fdd->f", R).real
    return R + (diag_load * tr / D + FLOOR)[:, None, None] * np.eye(D)


def solve(R, Pm, diag_load):
    """G (F, D, C) complex128 = R'^-1 P by Cholesky in float64, bad (F,) bool.  A bin whose R or P is not finite, or whose
    R' is not positive definite, or whose G is not finite in float32, gets G = 0 and bad = True."""
    R, Pm = np.asarray(R).astype(np.complex128), np.asarray(Pm).astype(np.complex128)
    F, D, Cn = Pm.shape
    G, bad = np.zeros((F, D, Cn), np.complex128), np.zeros(F, bool)
    for f in range(F):
        if not (np.isfinite(R[f]).all() and np.isfinite(Pm[f]).all()):
            bad[f] = True
            continue
        try:
            L = np.linalg.cholesky(load(R[f:f + 1], diag_load)[0])
        except np.linalg.LinAlgError:
            bad[f] = True
            continue
        g = np.linalg.solve(L.conj().T, np.linalg.solve(L, Pm[f]))
        with np.errstate(over="ignore"):
            if not np.isfinite(g.astype(np.complex64)).all():
                bad[f] = True
                continue
        G[f] = g
    return G, bad


def apply(Y, G, delay, dtype=np.float64):
    """X[c, t, f] = Y[c, t, f] - sum_d conj(G[f, d, c]) y~(t)[d]; a bin whose G is all zero is copied"""
    ct = np.complex64 if dtype == np.float32 else np.complex128
    Y = np.asarray(Y)
    Yc, G = Y.astype(ct), np.asarray(G).astype(ct)
    taps = G.shape[1] // Y.shape[0]
    X = Yc - np.einsum("ftd,fdc->ctf", stack_past(Yc, taps, delay), G.conj()).astype(ct)
    dead = ~G.any(axis=(1, 2))
    X[:, :, dead] = Yc[:, :, dead]
    return X


def wpe(Y, taps=10, delay=3, iterations=3, diag_load=1e-3, dtype=np.float64, weight=None):
    """Returns (X, bad): X of the last iteration, bad = a bin of any iteration passed through.  weight: None (the power of the
    previous iterate) or a fixed (N, F) array."""
    Y = np.asarray(Y)
    X = Y.astype(np.complex64 if dtype == np.float32 else np.complex128)
    bad = False
    for _ in range(iterations):
        lam = power(X, dtype) if weight is None else weight
        R, Pm = correlations(Y, lam, taps, delay, dtype)
        G, b = solve(R, Pm, diag_load)
        bad = bad or bool(b.any())
        if dtype == np.float32:
            G = G.astype(np.complex64)
        X = apply(Y, G, delay, dtype)
    return X, bad


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic late-reverberation scene: a gated complex Gaussian source convolved over frames, per bin and channel
# ---------------------------------------------------------------------------------------------------------------------
def scene(Cn=4, N=600, F=9, delay=3, seed=0, taps=80, decay=12.0, noise=0.0):
    """Returns (Y, E): the reverberant spectrum (C, N, F) complex128 and its early part (the first `delay` taps)."""
    r = np.random.RandomState(seed)
    s = (r.standard_normal((N, F)) + 1j * r.standard_normal((N, F))) / np.sqrt(2)
    s = s * (r.rand(N) < 0.5)[:, None]                      # every frame on or off
    h = (r.standard_normal((Cn, taps, F)) + 1j * r.standard_normal((Cn, taps, F))) * np.exp(-np.arange(taps) / decay)[None, :, None]
    Y = np.zeros((Cn, N, F), np.complex128)
    E = np.zeros((Cn, N, F), np.complex128)
    for l in range(min(taps, N)):
        term = h[:, l, None, :] * s[None, :N - l, :]
        Y[:, l:, :] += term
        if l < delay:
            E[:, l:, :] += term
    if noise:
        Y = Y + noise * (r.standard_normal(Y.shape) + 1j * r.standard_normal(Y.shape))
    return Y, E


def reduction_db(X, Y, E):
    """10 log10(||Y - E||^2 / ||X - E||^2)"""
    return 10.0 * np.log10((np.abs(Y - E) ** 2).sum() / (np.abs(X - E) ** 2).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests: name -> (C, taps, delay, N, F, diag_load, seed, zero frames)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "c1_k1_d1_n1_f3": (1, 1, 1, 1, 3, 1e-3, 1, ()),                       # N = delay = 1
    "c2_k2_d3_n3_f17": (2, 2, 3, 3, 17, 1e-3, 2, ()),                     # N = delay
    "c3_k5_d3_n4_f33": (3, 5, 3, 4, 33, 1e-3, 3, ()),                     # N = delay + 1
    "c1_k10_d1_n2_f3": (1, 10, 1, 2, 3, 1e-3, 4, ()),                     # N = delay + 1
    "c7_k10_d3_n97_f17": (7, 10, 3, 97, 17, 1e-3, 5, ()),                 # the default front end: D = 70, three tiles
    "c8_k10_d3_n300_f33": (8, 10, 3, 300, 33, 1e-3, 6, ()),               # D = 80, D + C = 88
    "c8_k10_d1_n33_f3": (8, 10, 1, 33, 3, 1e-3, 7, ()),                   # N < D
    "c2_k5_d3_n300_f257": (2, 5, 3, 300, 257, 1e-3, 8, ()),               # the usual bin count
    "c3_k2_d1_n97_f33_zero": (3, 2, 1, 97, 33, 1e-6, 9, (0, 1, 40, 41, 42, 96)),      # frames that are zero on every channel
    "c7_k5_d1_n33_f17": (7, 5, 1, 33, 17, 1e-3, 10, (5,)),                # D + C = 42: two tiles
    "c2_k2_d3_n1023_f3": (2, 2, 3, P - 1, 3, 1e-3, 11, ()),               # one frame short of a part
    "c2_k2_d3_n1024_f3": (2, 2, 3, P, 3, 1e-3, 12, ()),                   # one part exactly
    "c1_k5_d1_n1025_f3": (1, 5, 1, P + 1, 3, 1e-3, 13, ()),               # one frame into the second part
    "c3_k1_d3_n2049_f3": (3, 1, 3, 2 * P + 1, 3, 1e-3, 14, ()),           # three parts
}
# one ragged minibatch: common C, F, taps, delay
RAGGED = dict(C=3, taps=5, delay=3, F=17, diag_load=1e-3, frames=(97, 3, 300, 1100), seeds=(21, 22, 23, 24))
ITERATIONS = 3


def make_input(Cn, N, F, delay, seed, zero=()):
    """a reverberant scene with a little sensor noise, as complex64"""
    Y, _ = scene(Cn, N, F, delay, seed, taps=40, decay=6.0, noise=0.05)
    for t in zero:
        Y[:, t, :] = 0
    return Y.astype(np.complex64)


def case_input(name):
    Cn, taps, delay, N, F, dl, seed, zero = CASES[name]
    return make_input(Cn, N, F, delay, seed, zero)


def ragged_inputs():
    r = RAGGED
    return [make_input(r["C"], n, r["F"], r["delay"], s) for n, s in zip(r["frames"], r["seeds"])]


def integer_input(Cn, N, F, seed):
    """small integers, asymmetric across channels and frames, and weights that are 1 or a power of two: every product and
    every sum is exact in float32 (|entry| <= 2 * 4 * 4 * N * 4 < 2^24 for N <= 2^16)"""
    r = np.random.RandomState(seed)
    re = r.randint(-3, 5, size=(Cn, N, F)) + (np.arange(Cn) % 2)[:, None, None]
    im = r.randint(-4, 4, size=(Cn, N, F)) - (np.arange(N) % 2)[None, :, None]
    w = np.array([1.0, 0.5, 2.0, 0.25, 4.0], np.float32)[r.randint(0, 5, size=(N, F))]
    return (re + 1j * im).astype(np.complex64), w


def float32_errors():
    """The float32 mode against float64 over the very cases of the GPU tests, relative to max|want|: name -> dict(power,
    corr, apply, wpe).  This is where the tolerances of tests/test_gpu_wpe.py come from; run
    `python tests/wpe_ref.py` to print them."""
    out = {}
    items = [(n, case_input(n)) + CASES[n][1:3] + (CASES[n][5],) for n in CASES]
    items += [("ragged_%d" % n, y, RAGGED["taps"], RAGGED["delay"], RAGGED["diag_load"])
              for n, y in zip(RAGGED["frames"], ragged_inputs())]
    for name, Y, taps, delay, dl in items:
        lam = power(Y)
        e = dict(power=np.abs(power(Y, np.float32) - lam).max() / lam.max())
        lam32 = power(Y, np.float32)
        want, got = correlations(Y, lam32, taps, delay), correlations(Y, lam32, taps, delay, np.float32)
        e["corr"] = max(np.abs(g - w).max() / max(np.abs(w).max(), 1e-300) for g, w in zip(got, want))
        G = solve(*want, dl)[0].astype(np.complex64)
        X = apply(Y, G, delay)
        e["apply"] = np.abs(apply(Y, G, delay, np.float32) - X).max() / np.abs(X).max()
        full = wpe(Y, taps, delay, ITERATIONS, dl)[0]
        e["wpe"] = np.abs(wpe(Y, taps, delay, ITERATIONS, dl, np.float32)[0] - full).max() / np.abs(full).max()
        out[name] = e
    return out


if __name__ == "__main__":
    errs = float32_errors()
    for name, e in errs.items():
        print("%-24s %s" % (name, "  ".join("%s %.2e" % kv for kv in e.items())))
    for key in ("power", "corr", "apply", "wpe"):
        vals = [e[key] for e in errs.values()]
        print("%s: %.2e .. %.2e" % (key, min(vals), max(vals)))
