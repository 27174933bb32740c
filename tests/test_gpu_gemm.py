"""The pk2_gemm_f32 family (csrc/gemm_f32.hip; bf16x3 arithmetic: csrc/gemm_bf16x3.h) against oracle/gemm_ref.py.

  * Exact-integer operands (gemm_ref.exact_family): every correct kernel returns the float64 answer bit for bit, in any
    summation order; a dropped part product, a lo plane in the wrong place or an unsplit operand changes the result.
  * Poisoned memory: every operand sits inside a larger buffer of NaN -- a leading dimension beyond the row with NaN in the
    gap, NaN rows before and after, alternately a base one float off 16-byte alignment (the scalar loaders).  A read outside
    the logical matrix shows as NaN.  C sits in a buffer of SENTINEL: a write outside the M x N window changes it.  With
    beta = 0, C starts as NaN and must come back finite (the BLAS contract the models rely on with torch.empty outputs).
  * Every case runs on both arithmetic paths and under each schedule the per-call switches force (PK2_GEMM_TILES,
    PK2_GEMM_SPLITK, PK2_GEMM_BANDS are read on every call; PK2_GEMM_SPLIT_MID / _SPLIT_FWD / _BANDS_ONE / _FUSE_COLSUM
    once per process, so they are left alone).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import gemm_ref as G
from pykaldi2_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SCHEDULES = [{}, {"PK2_GEMM_TILES": "1"}, {"PK2_GEMM_TILES": "2"}, {"PK2_GEMM_SPLITK": "3"}, {"PK2_GEMM_SPLITK": "1"}]
SCALARS = [(1.0, 0.0, True), (2.0, 1.0, True), (-0.5, 2.0, False), (1.0, 0.5, True)]     # (alpha, beta, bias?)


def L():
    return _lib.lib()


def sp():
    return _lib.stream_ptr()


class Placed:
    """A [rows, cols] host matrix placed inside a device buffer of `fill`: leading dimension ld >= cols, `pre` / `post`
    rows of fill around it, base `off` floats into the buffer.  .ptr is the matrix's element (0, 0)."""

    def __init__(self, host, aligned, fill=float("nan"), pre=2, post=2, extra=0):
        host = np.asarray(host, np.float32)
        rows, cols = host.shape
        self.ld = (-(-cols // 4) * 4 + 4) if aligned else cols + 1
        self.off = (4 if aligned else 1) + pre * self.ld + extra
        self.buf = torch.full((self.off + (rows + post) * self.ld + 4,), fill, dtype=torch.float32)
        view = self.buf[self.off:self.off + rows * self.ld].view(rows, self.ld)
        view[:, :cols] = torch.from_numpy(host)
        self.rows, self.cols = rows, cols
        self.buf = self.buf.cuda()
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def window(self):
        b = self.buf.cpu()
        return b[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols].numpy()

    def outside(self):
        b = self.buf.cpu().clone()
        b[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = SENTINEL
        return b.numpy()


@functools.lru_cache(maxsize=None)
def family(fam, M, N, K, seed=0):
    return G.exact_family(fam, M, N, K, seed=seed + M * 7 + N * 13 + K)


def run_env(monkeypatch, env):
    for k in ("PK2_GEMM_TILES", "PK2_GEMM_SPLITK", "PK2_GEMM_BANDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_c(Cp, want):
    got = Cp.window()
    assert np.isfinite(got).all(), "non-finite outputs: a read outside an operand, or beta * C read with beta = 0"
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, ("%d of %d outputs differ, first at %s: %r != %r" %
                           (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
    assert (Cp.outside() == np.float32(SENTINEL)).all(), "a write outside the M x N window of C"


def place_c(C0, beta, aligned):
    C = Placed(C0 if beta != 0.0 else np.full(C0.shape, np.nan, np.float32), aligned, fill=SENTINEL)
    return C


def gemm_case(ta, tb, M, N, K, fam, alpha, beta, with_bias, aligned, seed=0):
    A, B = family(fam, M, N, K, seed)
    C0, bias = G.exact_extras(M, N, seed=seed + M + N, bias=with_bias)
    Ap = Placed(A.T if ta else A, aligned)
    Bp = Placed(B.T if tb else B, aligned)
    Cp = place_c(C0, beta, aligned)
    bp = Placed(bias[None, :], aligned) if bias is not None else None
    return A, B, C0, bias, Ap, Bp, Cp, bp


SHAPES = [(1, 1, 1), (2, 3, 17), (3, 5, 3), (5, 2, 256), (64, 64, 1030), (65, 129, 17), (129, 65, 256), (3, 129, 4100),
          (129, 1, 1030), (65, 64, 4100), (64, 5, 4100)]


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_exact_families_poisoned(M, N, K, ta, tb, arith, gemm_arith, monkeypatch):
    gemm_arith(arith)
    i = 0
    for env in SCHEDULES:
        run_env(monkeypatch, env)
        for fam in "abc":
            alpha, beta, with_bias = SCALARS[i % len(SCALARS)]
            aligned = i % 2 == 0
            i += 1
            A, B, C0, bias, Ap, Bp, Cp, bp = gemm_case(ta, tb, M, N, K, fam, alpha, beta, with_bias, aligned)
            _lib.check(L().pk2_gemm_f32(ta, tb, M, N, K, alpha, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld,
                                        bp.ptr if bp else None, sp()))
            check_c(Cp, G.gemm_exact(A, B, alpha, beta, C0, bias))


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("env", [{}, {"PK2_GEMM_BANDS": "0"}])
def test_gemm_exact_row_bands_and_scaled_rows(ta, tb, env, arith, gemm_arith, monkeypatch):
    """A product big enough for the row-band launch (a band of 128x128 tiles, the rest on 64x64 tiles), with power-of-two
    row and column scales up to 2^+-30 each (exact: each output is an integer times its own power of two)."""
    gemm_arith(arith)
    run_env(monkeypatch, env)
    M, N, K = 2200, 4096, 256
    rng = np.random.default_rng(ta * 2 + tb)
    re, ce = rng.integers(-30, 31, size=M), rng.integers(-30, 31, size=N)
    fam = "abc"[(2 * ta + tb) % 3]
    A, B = G.exact_family(fam, M, N, K, seed=4, row_exp=re, col_exp=ce)
    C0, _ = G.exact_extras(M, N, seed=4, row_exp=re, col_exp=ce)
    for beta, aligned in ((0.0, True), (1.0, False)):
        Ap, Bp = Placed(A.T if ta else A, aligned), Placed(B.T if tb else B, aligned)
        Cp = place_c(C0, beta, aligned)
        _lib.check(L().pk2_gemm_f32(ta, tb, M, N, K, 2.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld, None, sp()))
        check_c(Cp, G.gemm_exact(A, B, 2.0, beta, C0))


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(3, 5, 17), (65, 129, 1030), (129, 64, 256)])
def test_gemm_act_exact_poisoned(M, N, K, ta, tb, arith, gemm_arith, monkeypatch):
    """pk2_gemm_f32_act: ReLU (act 1) and the gate mask (act 2, gate with ldg > N in a NaN buffer)."""
    gemm_arith(arith)
    rng = np.random.default_rng(M + K)
    for env, fam in (({}, "a"), ({"PK2_GEMM_TILES": "1"}, "b"), ({"PK2_GEMM_TILES": "2"}, "c")):
        run_env(monkeypatch, env)
        for act in (1, 2):
            for alpha, beta, with_bias in SCALARS[:2]:
                A, B, C0, bias, Ap, Bp, Cp, bp = gemm_case(ta, tb, M, N, K, fam, alpha, beta, with_bias, act == 1)
                gate = rng.choice([-1.0, 0.0, 1.0], size=(M, N)).astype(np.float32)
                gp = Placed(gate, False)
                _lib.check(L().pk2_gemm_f32_act(ta, tb, M, N, K, alpha, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld,
                                                bp.ptr if bp else None, act, gp.ptr if act == 2 else None, gp.ld, sp()))
                want = G.gemm_exact(A, B, alpha, beta, C0, bias)
                want = np.maximum(want, 0.0) if act == 1 else np.where(gate > 0, want, 0.0)
                check_c(Cp, want)


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("M,N,K", [(5, 3, 17), (130, 65, 256), (64, 129, 1030)])
def test_gemm_seg_exact_poisoned(M, N, K, tb, sign, arith, gemm_arith, monkeypatch):
    """pk2_gemm_f32_seg, nseg = 3 over row-shifted views of one A buffer (segA = +-shift * lda, the Conv1d form) and three
    B slices (segB = +-their size, both signs); one segment stride not a multiple of four (scalar loaders)."""
    gemm_arith(arith)
    shift = 3
    fam = "c"
    Afull, _ = family(fam, M + 2 * shift, N, K, 1)
    Bs = [family(fam, M, N, K, 2 + j)[1] for j in range(3)]
    for env in ({}, {"PK2_GEMM_TILES": "1"}, {"PK2_GEMM_TILES": "2"}):
        run_env(monkeypatch, env)
        for aligned in (True, False):
            Ap = Placed(Afull, aligned)
            Bst = np.concatenate([(b.T if tb else b) for b in Bs[::sign]], 0)
            Bp = Placed(Bst, aligned)
            bsz = Bst.shape[0] // 3 * Bp.ld
            C0, bias = G.exact_extras(M, N, seed=M, bias=True)
            Cp = place_c(C0, 1.0, aligned)
            # segment j: A rows shift * (1 + sign * (j - 1)) ..., B slice j
            a0 = ctypes.c_void_p(Ap.ptr.value + 4 * (shift * (1 - sign)) * Ap.ld)
            b0 = ctypes.c_void_p(Bp.ptr.value + 4 * (0 if sign > 0 else 2 * bsz))
            bp = Placed(bias[None, :], aligned)
            _lib.check(L().pk2_gemm_f32_seg(0, tb, M, N, K, 3, 1.0, a0, Ap.ld, sign * shift * Ap.ld, b0, Bp.ld, sign * bsz, 1.0,
                                            Cp.ptr, Cp.ld, bp.ptr, 0, None, 0, sp()))
            want = C0.astype(np.float64) + bias
            for j in range(3):
                rows = shift * (1 - sign) + sign * shift * j
                want = want + G.gemm_exact(Afull[rows:rows + M], Bs[j])
            check_c(Cp, want)


def _batched_case(ta, tb, M, N, K, n0, n1, sA, sB, sC, fam, beta, seed):
    """Matrices of n0 x n1 batch entries in one NaN buffer per operand at offsets i0 sX[0] + i1 sX[1] from a base chosen so
    that every entry lies inside (strides may be zero or negative).  Returns host operands, device bases and buffers."""
    def place(shapes_host, s, ld, fill):
        offs = [i0 * s[0] + i1 * s[1] for i0 in range(n0) for i1 in range(n1)]
        rows, cols = shapes_host[0].shape
        lo = min(offs)
        span = max(offs) - lo + rows * ld
        base = 8 * ld + 1 - lo            # (one float off alignment: unless s and ld are multiples of 4, nothing is aligned)
        buf = np.full(base + lo + span + 8 * ld, fill, np.float32)
        for h, o in zip(shapes_host, offs):
            for r in range(rows):
                buf[base + o + r * ld:base + o + r * ld + cols] = h[r]
        t = torch.from_numpy(buf).cuda()
        return t, ctypes.c_void_p(t.data_ptr() + 4 * base), base
    As, Bs = [], []
    for z in range(n0 * n1):
        A, B = family(fam, M, N, K, seed + z)
        As.append(A)
        Bs.append(B)
    C0s = [G.exact_extras(M, N, seed=seed + z, bias=False)[0] for z in range(n0 * n1)]
    return As, Bs, C0s, place


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("strides", ["positive", "broadcast", "negative", "odd"])
def test_gemm_batched_exact_poisoned(ta, tb, strides, arith, gemm_arith):
    gemm_arith(arith)
    M, N, K, n0, n1 = 65, 33, 300, 2, 3
    ldA, ldB, ldC = (M if ta else K) + 3, (K if tb else N) + 5, N + 2
    szA, szB, szC = (K if ta else M) * ldA, (N if tb else K) * ldB, M * ldC
    sA, sB, sC = {"positive": ((n1 * szA, szA), (n1 * szB, szB), (n1 * szC, szC)),
                  "broadcast": ((0, szA), (0, 0), (n1 * szC, szC)),
                  "negative": ((-n1 * szA - 7, -szA), (n1 * szB + 10, -szB - 2), (-n1 * szC, -szC)),
                  "odd": ((n1 * szA + 5, szA + 1), (n1 * szB + 30, szB + 7), (n1 * szC + 11, szC + 3))}[strides]
    As, Bs, C0s, place = _batched_case(ta, tb, M, N, K, n0, n1, sA, sB, sC, "a" if tb else "b", 1.0, 11)
    # broadcast: entries that share an offset hold the same operand
    def uniq(mats, s):
        out = {}
        for z in range(n0 * n1):
            o = (z // n1) * s[0] + (z % n1) * s[1]
            out.setdefault(o, mats[z])
        return [out[(z // n1) * s[0] + (z % n1) * s[1]] for z in range(n0 * n1)]
    As, Bs = uniq(As, sA), uniq(Bs, sB)
    ta_h = [a.T if ta else a for a in As]
    tb_h = [b.T if tb else b for b in Bs]
    at, ap, _ = place(ta_h, sA, ldA, np.nan)
    bt, bp, _ = place(tb_h, sB, ldB, np.nan)
    for beta in (0.0, 1.0):
        ct, cp, cbase = place(C0s if beta else [np.full((M, N), np.nan, np.float32)] * (n0 * n1), sC, ldC, SENTINEL)
        _lib.check(L().pk2_gemm_f32_batched(ta, tb, M, N, K, 2.0, ap, ldA, sA[0], sA[1], bp, ldB, sB[0], sB[1], beta, cp, ldC,
                                            sC[0], sC[1], n0, n1, sp()))
        c = ct.cpu().numpy()
        seen = np.zeros(c.shape, bool)
        for z in range(n0 * n1):
            o = cbase + (z // n1) * sC[0] + (z % n1) * sC[1]
            got = np.stack([c[o + r * ldC:o + r * ldC + N] for r in range(M)])
            want = G.gemm_exact(As[z], Bs[z], 2.0, beta, C0s[z])
            assert np.array_equal(got.astype(np.float64), want), (z, beta, np.abs(got - want).max())
            for r in range(M):
                seen[o + r * ldC:o + r * ldC + N] = True
        assert (c[~seen] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
def test_gemm_batched_attention_shapes_exact(arith, gemm_arith):
    """The unfused attention's batched products (transformer.py: scores Q K^T over a [T, B, 3C] qkv buffer, lda = B * 3C;
    context P V; the dV form P^T dctx), n0 = utterances, n1 = heads."""
    gemm_arith(arith)
    T, Bu, H, d = 45, 3, 4, 16
    C = H * d
    rng = np.random.default_rng(0)
    qkv = np.zeros((T, Bu, 3 * C), np.float32)
    qkv[:, :, :C] = G._ints_with_planes(rng, T * Bu * C, 18, True).reshape(T, Bu, C)              # Q: dense 18-bit
    qkv[:, :, C:2 * C] = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], size=(T, Bu, C))                 # K: <= d = 16 per dot
    qkv[:, :, 2 * C:] = G._ints_with_planes(rng, T * Bu * C, 10, False).reshape(T, Bu, C)         # V: 10-bit
    P = np.zeros((Bu * H, T, T), np.float32)
    for z in range(Bu * H):
        for t in range(T):
            P[z, t, G.k_positions(T, rng, 4)] = G._ints_with_planes(rng, 4, 10, False)            # P: 4 per row
    q = torch.from_numpy(qkv).cuda()
    p = torch.from_numpy(P).cuda()
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)      # noqa: E731
    # scores: S[b, h] = Q_bh K_bh^T, Q_bh = qkv[:, b, h d:(h + 1) d]
    S = torch.full((Bu * H, T, T), float("nan"), device="cuda")
    _lib.check(L().pk2_gemm_f32_batched(0, 1, T, T, d, 0.5, ptr(q), Bu * 3 * C, 3 * C, d, ptr(q, C), Bu * 3 * C, 3 * C, d, 0.0,
                                        ptr(S), T, H * T * T, T * T, Bu, H, sp()))
    # context: cx[:, b, h d..] = P_bh V_bh
    cx = torch.full((T, Bu, C), float("nan"), device="cuda")
    _lib.check(L().pk2_gemm_f32_batched(0, 0, T, d, T, 1.0, ptr(p), T, H * T * T, T * T, ptr(q, 2 * C), Bu * 3 * C, 3 * C, d, 0.0,
                                        ptr(cx), Bu * C, C, d, Bu, H, sp()))
    # dV form: out[:, b, h d..] = P_bh^T K_bh (K: values of at most 2, so a column of P may hold any number of non-zeros)
    dv = torch.full((T, Bu, C), float("nan"), device="cuda")
    _lib.check(L().pk2_gemm_f32_batched(1, 0, T, d, T, 1.0, ptr(p), T, H * T * T, T * T, ptr(q, C), Bu * 3 * C, 3 * C, d, 0.0,
                                        ptr(dv), Bu * C, C, d, Bu, H, sp()))
    S, cx, dv = S.cpu().numpy(), cx.cpu().numpy(), dv.cpu().numpy()
    for b in range(Bu):
        for h in range(H):
            Q = qkv[:, b, h * d:(h + 1) * d]
            Kh = qkv[:, b, C + h * d:C + (h + 1) * d]
            V = qkv[:, b, 2 * C + h * d:2 * C + (h + 1) * d]
            Pz = P[b * H + h]
            assert np.array_equal(S[b * H + h].astype(np.float64), G.gemm_exact(Q, Kh.T, 0.5)), (b, h)
            assert np.array_equal(cx[:, b, h * d:(h + 1) * d].astype(np.float64), G.gemm_exact(Pz, V)), (b, h)
            assert np.array_equal(dv[:, b, h * d:(h + 1) * d].astype(np.float64), G.gemm_exact(Pz.T, Kh)), (b, h)


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("M,N,K", [(1, 3, 17), (5, 64, 256), (65, 129, 1030), (130, 70, 4100), (3, 2, 4100)])
@pytest.mark.parametrize("env", [{}, {"PK2_GEMM_SPLITK": "3"}, {"PK2_GEMM_TILES": "1"}])
def test_gemm_tn_colsum_exact_poisoned(M, N, K, env, arith, gemm_arith, monkeypatch):
    """pk2_gemm_f32_tn_colsum: C = alpha A^T B + beta C and colsum += the column sums of A ([K, M] in a NaN buffer), both
    exact; then pk2_colsum_f32 alone with beta = 0 must ignore a NaN out."""
    gemm_arith(arith)
    run_env(monkeypatch, env)
    At, B = family("b", M, N, K, 3)                      # A^T [M, K]: sparse {0, +-1, +-2} -> exact column sums
    A = At.T.copy()
    for aligned, beta in ((True, 1.0), (False, 0.0)):
        C0, _ = G.exact_extras(M, N, seed=K, bias=False)
        cs0 = np.arange(M, dtype=np.float32) % 7 - 3
        Ap, Bp, Cp = Placed(A, aligned), Placed(B, aligned), place_c(C0, beta, aligned)
        csp = Placed(cs0[None, :], aligned, fill=SENTINEL)
        _lib.check(L().pk2_gemm_f32_tn_colsum(M, N, K, 2.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld, csp.ptr, sp()))
        check_c(Cp, G.gemm_exact(At, B, 2.0, beta, C0))
        check_c(csp, A.astype(np.float64).sum(0)[None, :] + cs0)
        out = Placed(np.full((1, M), np.nan, np.float32), aligned, fill=SENTINEL)
        _lib.check(L().pk2_colsum_f32(Ap.ptr, Ap.ld, K, M, 0.0, out.ptr, sp()))
        check_c(out, A.astype(np.float64).sum(0)[None, :])
        _lib.check(L().pk2_colsum_f32(Ap.ptr, Ap.ld, K, M, 0.5, out.ptr, sp()))
        check_c(out, 1.5 * A.astype(np.float64).sum(0)[None, :])


# ---------------------------------------------------------------- random data: err_units bound
STAT_CASES = [("act_w", 2276, 512, 1024), ("act_w", 300, 4096, 64), ("normal", 129, 65, 256), ("normal", 1000, 700, 1024),
              ("wgrad", 512, 512, 20480), ("normal", 130, 70, 4100)]


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("kind,M,N,K", STAT_CASES)
def test_gemm_error_bound_random_data(kind, M, N, K, arith, gemm_arith):
    """err_units of the device product on the models' value distributions (gemm_ref.random_case), every layout, some rows and
    columns scaled by 2^+-100 (judged against their own sum |a b|).  Bounds: gemm_ref.STAT_BOUND, rms / max -- bf16x3
    5.5e-8 / 6.5e-7, f32 6e-8 / 6.5e-7.  Measured on an MI355X (worst over layouts): f32 rms 2.5-2.8e-8, max 2.0-3.1e-7;
    bf16x3 rms 1.9-2.5e-8, max 1.5-2.8e-7.  Every CPU mutation of the split has rms >= 1.1e-7 at K <= 1024
    (tests/test_gemm_ref.py)."""
    gemm_arith(arith)
    A, B = G.random_case(kind, M, N, K, seed=M + K)
    rng = np.random.default_rng(K)
    re = np.where(rng.random(M) < 0.1, rng.choice([-100, 100], size=M), 0)
    ce = np.where(rng.random(N) < 0.1, rng.choice([-100, 100], size=N), 0)
    ce = np.where(re.max() + ce > 120, 0, ce)
    ce = np.where(re.min() + ce < -120, 0, ce)
    A = np.ldexp(A, re[:, None].astype(np.int32)).astype(np.float32)
    B = np.ldexp(B, ce[None, :].astype(np.int32)).astype(np.float32)
    rms_b, max_b = G.STAT_BOUND[arith]
    worst = (0.0, 0.0)
    for ta, tb in ((0, 1), (0, 0), (1, 0), (1, 1)):
        a = torch.from_numpy(A.T.copy() if ta else A).cuda()
        b = torch.from_numpy(B.T.copy() if tb else B).cuda()
        c = torch.full((M, N), float("nan"), device="cuda")
        _lib.check(L().pk2_gemm_f32(ta, tb, M, N, K, 1.0, _lib.ptr(a), a.shape[1], _lib.ptr(b), b.shape[1], 0.0, _lib.ptr(c), N,
                                    None, sp()))
        rms, mx = G.err_units(c.cpu().numpy(), A, B)
        print("%s %s %dx%dx%d ta=%d tb=%d: err_units rms %.3g max %.3g" % (arith, kind, M, N, K, ta, tb, rms, mx))
        worst = (max(worst[0], rms), max(worst[1], mx))
        assert rms <= rms_b and mx <= max_b, (ta, tb, rms, mx)
    print("MEASURED %s %s %dx%dx%d worst rms %.3g max %.3g" % ((arith, kind, M, N, K) + worst))


# ---------------------------------------------------------------- subnormal edge of the split
SUB_EXPS = list(range(-120, -151, -1))


def _subnormal_exact(s, ta, tb):
    """Family a (A 18-bit integers: hi, mid and lo planes) with A scaled by 2^s, B by 2^120: is the device product exact?"""
    M, N, K = 33, 40, 64
    A, B = family("a", M, N, K, 9)
    A = np.ldexp(A, s).astype(np.float32)
    B = np.ldexp(B, 120).astype(np.float32)          # (products 2^(s + 120) times integers: normal)
    a = torch.from_numpy(A.T.copy() if ta else A).cuda()
    b = torch.from_numpy(B.T.copy() if tb else B).cuda()
    c = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(L().pk2_gemm_f32(ta, tb, M, N, K, 1.0, _lib.ptr(a), a.shape[1], _lib.ptr(b), b.shape[1], 0.0, _lib.ptr(c), N,
                                None, sp()))
    got = c.cpu().numpy().astype(np.float64)
    want = G.gemm_exact(A, B)
    # the documented bound below 2^-110: each element of A off by at most 2^-134 (plus the f32 rounding of the sum)
    lim = np.abs(B.astype(np.float64)).sum(0)[None, :] * 2.0 ** -134 + np.abs(want) * 2.0 ** -22
    return bool(np.array_equal(got, want)), bool((np.abs(got - want) <= lim).all()), bool(np.isfinite(got).all())


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
def test_gemm_subnormal_edge(arith, gemm_arith):
    """Where the bf16x3 split stops being exact (documented in gemm_bf16x3.h).  A = 18-bit integers times 2^s: its lowest
    bits sit in the lo plane at 2^s.  Measured on an MI355X: exact for s >= -133 (the lo plane down to 2^-133, the smallest
    bf16 subnormal: neither the split's conversion nor the bf16 MFMA flushes), inexact from s = -134 on with a graceful loss
    (largest relative error 5e-6 at s = -134, 2e-4 at -140, 0.19 at -150).  The f32 path is exact over the whole range
    (subnormal f32 operands included)."""
    gemm_arith(arith)
    for s in SUB_EXPS:
        for ta, tb in ((0, 1), (1, 0)):
            exact, within, finite = _subnormal_exact(s, ta, tb)
            assert finite and within, (s, ta, tb)
            assert exact == (arith == "f32" or s >= -133), (s, ta, tb, exact)


# ---------------------------------------------------------------- f32 mode against a k-ordered fmaf chain
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f32_against_fmaf_chain(ta, tb, gemm_arith):
    gemm_arith("f32")
    M, N, K = 32, 32, 64
    A, B = G.random_case("normal", M, N, K, seed=3)
    a = torch.from_numpy(A.T.copy() if ta else A).cuda()
    b = torch.from_numpy(B.T.copy() if tb else B).cuda()
    c = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(L().pk2_gemm_f32(ta, tb, M, N, K, 1.0, _lib.ptr(a), a.shape[1], _lib.ptr(b), b.shape[1], 0.0, _lib.ptr(c), N,
                                None, sp()))
    got = c.cpu().numpy()
    chain, serial = G.fmaf_chain(A, B), G.serial_f32(A, B)
    print("FMAF ta=%d tb=%d: differs from fmaf chain in %d, from serial in %d of %d; err_units %s chain %s" %
          (ta, tb, (got != chain).sum(), (got != serial).sum(), got.size, G.err_units(got, A, B), G.err_units(chain, A, B)))
    assert np.array_equal(got, chain)
