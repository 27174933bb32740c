"""Host reference for the pk2_gemm_f32 family (csrc/gemm_f32.hip, csrc/gemm_bf16x3.h).  CPU only, numpy / torch.

  * split3 / x3_product: the bf16x3 arithmetic -- every f32 operand element split into three bf16 planes, six of the nine
    part products kept -- with named MUTATIONS (a dropped part product, a zeroed lo plane, no split at all), so the tests
    can show that a check tells a correct kernel from a broken one.
  * fmaf / fmaf_chain: an exact emulation of a k-ordered float32 fmaf chain (one rounding per product).
  * exact_family: operands whose part products and every partial sum are integers below 2^24 (times per-row / per-column
    powers of two), so that any correct kernel returns the float64 answer bit for bit in any summation order, split-K
    float atomics included, while each mutation changes the result.
  * err_units: the error of every element in units of sum_k |alpha a b| + |beta C| + |bias|.
"""
import numpy as np
import torch

MUTATIONS = ("drop_hl", "drop_lh", "drop_mm", "zero_lo_a", "zero_lo_b", "hi_only")
SLAB = (16, 32)                 # k-slab depths of the kernels (f32 and 128x128 bf16x3 tiles: 16; 64x64 bf16x3 tiles: 32)


def bf16_rne(x):
    """float32 -> nearest bf16 (ties to even), returned as float32.  Subnormals are kept (no flush)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = hi + mid + lo exactly, as gemm_bf16x3.h:2 defines it: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
    each difference formed in float32."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    lo = bf16_rne((r - mid).astype(np.float32))
    return hi, mid, lo


def x3_product(A, B, mutation=None):
    """A [M, K] @ B [K, N] (float32, logical layout) in the kernel's arithmetic: the six kept part products, each exact in
    float32, summed in float32 in the kernel's order (small terms first).  `mutation`: one of MUTATIONS, or None."""
    ah, am, al = split3(A)
    bh, bm, bl = split3(B)
    if mutation == "zero_lo_a":
        al = np.zeros_like(al)
    if mutation == "zero_lo_b":
        bl = np.zeros_like(bl)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))      # noqa: E731
    ah, am, al, bh, bm, bl = (t(v) for v in (ah, am, al, bh, bm, bl))
    z = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    if mutation == "hi_only":
        return (ah @ bh).numpy()
    lh = z if mutation == "drop_lh" else al @ bh
    hl = z if mutation == "drop_hl" else ah @ bl
    mm = z if mutation == "drop_mm" else am @ bm
    return ((((lh + hl) + mm) + (am @ bh + ah @ bm)) + ah @ bh).numpy()


def gemm_exact(A, B, alpha=1.0, beta=0.0, C0=None, bias=None):
    """alpha A B + beta C0 + bias in float64 (A [M, K], B [K, N] logical)."""
    want = alpha * (np.asarray(A, np.float64) @ np.asarray(B, np.float64))
    if beta != 0.0:
        want = want + beta * np.asarray(C0, np.float64)
    if bias is not None:
        want = want + np.asarray(bias, np.float64)[None, :]
    return want


def err_units(got, A, B, alpha=1.0, beta=0.0, C0=None, bias=None, want=None):
    """|got - exact| per element over sum_k |alpha a_mk b_kn| + |beta C0_mn| + |bias_n|  ->  (rms, max) over elements.
    An element whose unit is zero counts as 0 when exact and inf otherwise.  `want`: the exact answer when it is not the
    plain product (e.g. behind a ReLU, which does not widen the error)."""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if want is None:
        want = gemm_exact(A64, B64, alpha, beta, C0, bias)
    unit = abs(alpha) * (np.abs(A64) @ np.abs(B64))
    if beta != 0.0:
        unit = unit + abs(beta) * np.abs(np.asarray(C0, np.float64))
    if bias is not None:
        unit = unit + np.abs(np.asarray(bias, np.float64))[None, :]
    e = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, e / np.where(unit > 0, unit, 1.0), np.where(e == 0, 0.0, np.inf))
    return float(np.sqrt(np.mean(r * r))), float(r.max())


# ---------------------------------------------------------------- exact float32 fmaf
def fmaf(a, b, c):
    """Correctly rounded float32 a * b + c (elementwise, normal range).  a * b is exact in float64; the float64 sum's own
    error (TwoSum) decides the one case where rounding the float64 sum to float32 is not the rounding of the exact sum: a
    float64 sum that lies exactly halfway between two float32 numbers."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                    # exact: p + c = s + e
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    away = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf))).astype(np.float32)
    tie = (e != 0) & (s != r64) & (s == 0.5 * (r64 + away.astype(np.float64)))
    # at a tie the exact sum lies on e's side of s
    toward_away = np.sign(e) == np.sign(away.astype(np.float64) - s)
    return np.where(tie & toward_away, away, r).astype(np.float32)


def fmaf_chain(A, B):
    """C[m, n] = fmaf(a_{K-1} b_{K-1}, ... fmaf(a_0, b_0, 0)): the k-ordered float32 fmaf chain (A [M, K], B [K, N])."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = fmaf(A[:, k:k + 1], B[k:k + 1, :], acc)
    return acc


def serial_f32(A, B):
    """The same k-ordered chain with a rounded product and a rounded sum (two roundings per k)."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc + (A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    return acc


# ---------------------------------------------------------------- exact-integer fixtures
def _ints_with_planes(rng, n, bits, need_lo):
    """n signed integers of exactly `bits` significant bits whose split has a non-zero mid plane, and a non-zero (need_lo)
    or zero (not need_lo) lo plane."""
    assert bits >= (18 if need_lo else 10)
    out = np.empty(0, np.float32)
    while out.size < n:
        v = (rng.integers(1 << (bits - 1), 1 << bits, size=4 * n + 64) * rng.choice([-1, 1], size=4 * n + 64)).astype(np.float32)
        _, m, lo = split3(v)
        ok = (m != 0) & ((lo != 0) if need_lo else (lo == 0))
        out = np.concatenate([out, v[ok]])
    return out[:n]


def k_positions(K, rng, n):
    """n distinct k indices (fewer if K < n): k = 0, K - 1, both sides of the 16 / 32 slab boundaries, the partial last slab,
    the rest at random."""
    cand = {0, K - 1}
    for s in SLAB:
        for b in range(s, K, s):
            cand.update((b - 1, b))
        cand.update(range((K // s) * s, K))          # the partial last slab
    cand = np.array(sorted(c for c in cand if 0 <= c < K))
    n = min(n, K)
    must = np.array([0, K - 1])[:n]
    rest = rng.choice(cand, size=min(len(cand), n), replace=False)
    pick = list(dict.fromkeys(list(must) + list(rest)))
    if len(pick) < n:
        extra = rng.choice(np.setdiff1d(np.arange(K), pick), size=n - len(pick), replace=False)
        pick += list(extra)
    return np.array(pick[:n], np.int64)


def exact_family(fam, M, N, K, seed=0, row_exp=None, col_exp=None):
    """Operands (A [M, K], B [K, N], float32, logical layout) of family 'a', 'b' or 'c' (see the module docstring):
      a: A dense 18-bit integers (hi, mid and lo non-zero: 17 bits leave lo zero), B in {0, +-1, +-2} with at most 16
         non-zeros per column
         -> needs lo*hi;
      b: the mirror (A sparse rows of {0, +-1, +-2}, B dense 18-bit) -> needs hi*lo;
      c: 10-bit integers (hi and mid non-zero, lo zero), at most 4 non-zeros per dot product -> needs hh, hm, mh, mm.
    The non-zeros of the sparse operand sit at k_positions().  row_exp [M] / col_exp [N]: integer powers of two applied to
    the rows of A / the columns of B (|row_exp + col_exp| <= 60).  Asserts that sum_k |a b| < 2^24 in units of
    2^(row_exp + col_exp), i.e. that every partial sum of every output is exact in float32."""
    rng = np.random.default_rng(seed)
    dense_bits, nnz, need_lo = (18, 16, True) if fam in ("a", "b") else (10, 4, False)
    if fam == "c":
        A = _ints_with_planes(rng, M * K, 10, False).reshape(M, K)
        B = np.zeros((K, N), np.float32)
        for n in range(N):
            ks = k_positions(K, rng, nnz)
            B[ks, n] = _ints_with_planes(rng, len(ks), 10, False)
    else:
        dense_rows, sparse_cols = (M, N) if fam == "a" else (N, M)
        D = _ints_with_planes(rng, dense_rows * K, dense_bits, need_lo).reshape(dense_rows, K)
        S = np.zeros((K, sparse_cols), np.float32)
        for n in range(sparse_cols):
            ks = k_positions(K, rng, nnz)
            S[ks, n] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(ks))
        A, B = (D, S) if fam == "a" else (S.T.copy(), D.T.copy())
    bound = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64))
    assert bound.max() < 2.0 ** 23, bound.max()        # (2^23: room for alpha = 2 and beta C + bias within 2^24)
    if row_exp is not None or col_exp is not None:
        re = np.zeros(M, np.int64) if row_exp is None else np.asarray(row_exp, np.int64)
        ce = np.zeros(N, np.int64) if col_exp is None else np.asarray(col_exp, np.int64)
        assert np.abs(re[:, None] + ce[None, :]).max() <= 60
        A = np.ldexp(A, re[:, None].astype(np.int32)).astype(np.float32)
        B = np.ldexp(B, ce[None, :].astype(np.int32)).astype(np.float32)
    return A, B


def exact_extras(M, N, seed=0, row_exp=None, col_exp=None, bias=True):
    """C0 [M, N] of small integers (scaled like the product's element: 2^(row_exp + col_exp)) and, unless the rows are
    scaled, bias [N] of small integers."""
    rng = np.random.default_rng(seed + 7)
    C0 = rng.integers(-8, 9, size=(M, N)).astype(np.float32)
    if row_exp is not None or col_exp is not None:
        re = np.zeros(M, np.int32) if row_exp is None else np.asarray(row_exp, np.int32)
        ce = np.zeros(N, np.int32) if col_exp is None else np.asarray(col_exp, np.int32)
        C0 = np.ldexp(C0, re[:, None] + ce[None, :]).astype(np.float32)
        bias = bias and row_exp is None
        b = np.ldexp(rng.integers(-8, 9, size=N).astype(np.float32), ce).astype(np.float32) if bias else None
        return C0, b
    return C0, (rng.integers(-8, 9, size=N).astype(np.float32) if bias else None)


# ---------------------------------------------------------------- the models' value distributions
def random_case(kind, M, N, K, seed=0):
    """A [M, K], B [K, N] float32 with the value distributions of tools/bf16x3_error_study.py:
      'act_w':  tanh * sigmoid activations x U(-1/sqrt(H), 1/sqrt(H)) weights (H = 512) -- forward products;
      'normal': N(0, 1) x N(0, 1);
      'wgrad':  dY^T X of a weight gradient -- dY ~ N(0, 1e-3^2), X activations (K = frames)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "act_w":
        A = torch.tanh(torch.randn(M, K, generator=g)) * torch.sigmoid(torch.randn(M, K, generator=g))
        B = (torch.rand(K, N, generator=g) * 2 - 1) / 512 ** 0.5
    elif kind == "normal":
        A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    elif kind == "wgrad":
        A = torch.randn(M, K, generator=g) * 1e-3
        B = torch.tanh(torch.randn(K, N, generator=g)) * torch.sigmoid(torch.randn(K, N, generator=g))
    else:
        raise ValueError(kind)
    return A.numpy(), B.numpy()


# ---------------------------------------------------------------- statistical bound (err_units, random data)
# Bounds on (rms, max) of err_units per arithmetic, on 128 x 128 .. 2276 x 512 outputs of the random_case distributions.
#   CPU models, K = 64 .. 1024: the k-ordered fmaf chain (what the f32 path is) rms <= 2.9e-8, max <= 2.7e-7; the bf16x3 model
#   (each part product summed on its own) rms <= 1.1e-8; every MUTATION rms >= 1.1e-7, max >= 4.6e-7.
#   Device (MI355X, tests/test_gpu_gemm.py::test_gemm_error_bound_random_data, K = 64 .. 20480, all layouts, rows scaled by
#   2^+-100): f32 rms <= 2.82e-8, max <= 3.07e-7; bf16x3 rms <= 2.53e-8, max <= 2.76e-7 -- the six products share ONE
#   accumulator that rounds once per MFMA, six times per 16 k's, so the device error is 2x the model's.
# Both rms bounds sit 2x above the worst correct case and below every mutation at K <= 1024; the max bounds sit 2x above the
# worst correct case and catch an unsplit operand, but not a single dropped plane (its max is within 1.5x of the f32 chain's).
# At K = 4096 the mutations fall to rms 6e-8 (they shrink as 1 / sqrt(K)): no separation is claimed there.
STAT_BOUND = {"bf16x3": (5.5e-8, 6.5e-7), "f32": (6e-8, 6.5e-7)}
