"""The row-mapped products (pk2_gemm_f32_rows, pk2_gemm_f32_tn_colsum_rows, pk2_rows_zero, pk2_rows_pack; csrc/gemm_f32.hip)
on time-major [T * B, .] matrices whose padded rows hold NaN in EVERY input operand: one read of a padded row shows in
the result.  Both arithmetic paths.

  * forward (x W^T + b) and dX (dY W) form: the valid rows are bit-equal to the same rows of the unmapped product on
    random data (per element the k order is the unmapped kernel's whatever tiles the launch logic picks for Mv rows), exact
    on gemm_ref.exact_family operands in every schedule (K slices with float atomics included), the padded rows of C are
    not written by the product and exactly 0 behind pk2_rows_zero;
  * weight-gradient form: C and colsum equal gemm_ref.gemm_exact (float64) bit for bit on exact families -- that file's
    tolerance for them is zero -- with and without the K-slice rule engaged, aligned (vector loader) and unaligned (general
    loader) operands; pk2_rows_pack + the unmapped entry give the same;
  * the identity map (Mv == rows, or a null map) gives the unmapped entry's bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import gemm_ref as G
from pykaldi2_amd import _lib
from pykaldi2_amd.lstm import row_map_host

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
# (T, B, lengths): 11 valid rows of 21 (not a multiple of 4); 4 of 21; 172 of 280 (a second, partial 128-row tile)
BATCHES = [(7, 3, (7, 3, 1)), (7, 3, (2, 1, 1)), (70, 4, (70, 33, 5, 64))]
N_OUT, K_IN = 136, 72            # one 128-tile plus 8 columns; K = four f32 slabs and a half
ARITH = ["f32", "bf16x3"]


def L():
    return _lib.lib()


def sp():
    return _lib.stream_ptr()


def iptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


class Placed:
    """A [rows, cols] host matrix inside a device buffer of `fill`, leading dimension > cols, base 16-byte aligned or not."""

    def __init__(self, host, aligned, fill=float("nan")):
        host = np.asarray(host, np.float32)
        rows, cols = host.shape
        self.ld = (-(-cols // 4) * 4 + 4) if aligned else cols + 1
        self.off = (4 if aligned else 1) + 2 * self.ld
        buf = torch.full((self.off + (rows + 2) * self.ld + 4,), fill, dtype=torch.float32)
        buf[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, :cols] = torch.from_numpy(host)
        self.rows, self.cols = rows, cols
        self.buf = buf.cuda()
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def window(self):
        b = self.buf.cpu()
        return b[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols].numpy()

    def outside_untouched(self, fill):
        b = self.buf.cpu().clone()
        b[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = float(fill)
        return bool((b == float(fill)).all())


def scatter(valid_rows, rows, perm, mv, fill=np.nan):
    """[Mv, cols] -> [rows, cols] with the valid rows at perm[:mv] and `fill` in the padded rows."""
    full = np.full((rows, valid_rows.shape[1]), fill, np.float32)
    full[perm[:mv]] = valid_rows
    return full


@functools.lru_cache(maxsize=None)
def batch(T, B, lengths):
    perm, mv = row_map_host(lengths, T, B)
    return perm, mv, torch.from_numpy(perm).cuda()


def set_env(monkeypatch, env):
    for k in ("PK2_GEMM_TILES", "PK2_GEMM_SPLITK", "PK2_GEMM_BANDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def exact_equal(got, want, what):
    assert np.isfinite(got).all(), what + ": non-finite outputs (a padded row was read)"
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %s: %r != %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                          want[tuple(bad[0])])


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("T,B,lengths", BATCHES)
@pytest.mark.parametrize("tb", [1, 0])
def test_rows_forward_and_dx_bit_equal_to_unmapped(T, B, lengths, tb, arith, gemm_arith, monkeypatch):
    gemm_arith(arith)
    set_env(monkeypatch, {})
    perm, mv, dperm = batch(T, B, lengths)
    rows = T * B
    A, Bm = G.random_case("normal", mv, N_OUT, K_IN, seed=rows + tb)
    bias = np.linspace(-1, 1, N_OUT).astype(np.float32) if tb else None
    for aligned in (True, False):
        Ap = Placed(scatter(A, rows, perm, mv), aligned)
        Bp = Placed(Bm.T.copy() if tb else Bm, aligned)
        bp = Placed(bias[None, :], aligned) if bias is not None else None
        ref = Placed(np.full((rows, N_OUT), np.nan, np.float32), aligned, fill=SENTINEL)
        _lib.check(L().pk2_gemm_f32(0, tb, rows, N_OUT, K_IN, 1.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, 0.0, ref.ptr, ref.ld,
                                    bp.ptr if bp else None, sp()))
        Cp = Placed(np.full((rows, N_OUT), SENTINEL, np.float32), aligned, fill=SENTINEL)
        _lib.check(L().pk2_gemm_f32_rows(tb, rows, N_OUT, K_IN, 1.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, 0.0, Cp.ptr, Cp.ld,
                                         bp.ptr if bp else None, iptr(dperm), mv, sp()))
        got, want = Cp.window(), ref.window()
        assert np.isfinite(got[perm[:mv]]).all(), "a padded row of A was read"
        assert np.array_equal(got[perm[:mv]].view(np.uint32), want[perm[:mv]].view(np.uint32)), "valid rows differ from the unmapped product"
        assert (got[perm[mv:]] == np.float32(SENTINEL)).all(), "the product wrote a padded row of C"
        _lib.check(L().pk2_rows_zero(Cp.ptr, Cp.ld, N_OUT, iptr(dperm, mv), rows - mv, sp()))
        got = Cp.window()
        assert np.array_equal(got[perm[:mv]].view(np.uint32), want[perm[:mv]].view(np.uint32))
        assert (got[perm[mv:]].view(np.uint32) == 0).all(), "padded rows are not exactly +0"
        assert Cp.outside_untouched(np.float32(SENTINEL)), "a write outside the window of C"


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("T,B,lengths", BATCHES)
@pytest.mark.parametrize("env", [{}, {"PK2_GEMM_TILES": "1"}, {"PK2_GEMM_TILES": "2"}])
def test_rows_forward_and_dx_exact_in_every_schedule(T, B, lengths, env, arith, gemm_arith, monkeypatch):
    """Exact-integer operands: alpha, beta C and bias through the map, on 64x64 and on 128x128 tiles."""
    gemm_arith(arith)
    set_env(monkeypatch, env)
    perm, mv, dperm = batch(T, B, lengths)
    rows = T * B
    for tb, fam, alpha, beta, with_bias, aligned in ((1, "a", 1.0, 0.0, True, True), (0, "b", 2.0, 1.0, True, False),
                                                     (0, "c", -0.5, 2.0, False, True)):
        A, Bm = G.exact_family(fam, mv, N_OUT, K_IN, seed=rows + tb)
        C0, bias = G.exact_extras(mv, N_OUT, seed=rows, bias=with_bias)
        Ap = Placed(scatter(A, rows, perm, mv), aligned)
        Bp = Placed(Bm.T.copy() if tb else Bm, aligned)
        bp = Placed(bias[None, :], aligned) if bias is not None else None
        Cp = Placed(scatter(C0, rows, perm, mv, SENTINEL) if beta != 0.0 else np.full((rows, N_OUT), SENTINEL, np.float32), aligned,
                    fill=SENTINEL)
        _lib.check(L().pk2_gemm_f32_rows(tb, rows, N_OUT, K_IN, alpha, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld,
                                         bp.ptr if bp else None, iptr(dperm), mv, sp()))
        got = Cp.window()
        exact_equal(got[perm[:mv]], G.gemm_exact(A, Bm, alpha, beta, C0, bias), "tb=%d %s" % (tb, fam))
        assert (got[perm[mv:]] == np.float32(SENTINEL)).all() and Cp.outside_untouched(np.float32(SENTINEL))


@pytest.mark.parametrize("arith", ARITH)
def test_rows_row_bands_bit_equal_to_unmapped(arith, gemm_arith, monkeypatch):
    """2276 valid rows of 2800, N = 4096, K = 256: 18 x 32 tiles of 128 x 128 -- the size at which the launch logic cuts the
    mapped rows into a band of 128 x 128 tiles and a rest of 64 x 64 tiles in one launch (the bench's output layer)."""
    gemm_arith(arith)
    set_env(monkeypatch, {})
    T, B, lengths, N, K = 700, 4, (700, 600, 500, 476), 4096, 256
    perm, mv, dperm = batch(T, B, lengths)
    rows = T * B
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(rows, K, device="cuda", generator=g)
    a[torch.from_numpy(perm[mv:].astype(np.int64)).cuda()] = float("nan")
    w = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    valid = torch.from_numpy(perm[:mv].astype(np.int64)).cuda()
    for tb, bmat, ldb in ((1, w, K), (0, w.view(K, N), N)):
        ref = torch.empty(rows, N, device="cuda")
        _lib.check(L().pk2_gemm_f32(0, tb, rows, N, K, 1.0, _lib.ptr(a), K, _lib.ptr(bmat), ldb, 0.0, _lib.ptr(ref), N, _lib.ptr(bias), sp()))
        c = torch.full((rows, N), SENTINEL, device="cuda")
        _lib.check(L().pk2_gemm_f32_rows(tb, rows, N, K, 1.0, _lib.ptr(a), K, _lib.ptr(bmat), ldb, 0.0, _lib.ptr(c), N, _lib.ptr(bias),
                                         iptr(dperm), mv, sp()))
        _lib.check(L().pk2_rows_zero(_lib.ptr(c), N, N, iptr(dperm, mv), rows - mv, sp()))
        assert bool(torch.isfinite(c).all()), "a padded row of A was read"
        assert torch.equal(c[valid].view(torch.int32), ref[valid].view(torch.int32))
        assert int(c.view(torch.int32)[torch.from_numpy(perm[mv:].astype(np.int64)).cuda()].abs().max()) == 0


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("T,B,lengths", [BATCHES[0], BATCHES[2]])
def test_rows_dx_k_sliced_through_the_map(T, B, lengths, arith, gemm_arith, monkeypatch):
    """K = 1600 on two (four) tiles: the dX form is cut into K slices -- beta C + bias is applied to the MAPPED rows by the
    prescale launch, the slices add with float atomics into them (exact on these operands in any order); the forward form
    with the same K is never sliced."""
    gemm_arith(arith)
    set_env(monkeypatch, {})
    perm, mv, dperm = batch(T, B, lengths)
    rows, K = T * B, 1600
    for tb, beta in ((0, 0.0), (0, 2.0), (1, 1.0)):
        A, Bm = G.exact_family("b", mv, N_OUT, K, seed=rows + tb)
        C0, bias = G.exact_extras(mv, N_OUT, seed=rows, bias=True)
        Ap = Placed(scatter(A, rows, perm, mv), True)
        Bp = Placed(Bm.T.copy() if tb else Bm, True)
        bp = Placed(bias[None, :], True)
        Cp = Placed(scatter(C0, rows, perm, mv, SENTINEL) if beta != 0.0 else np.full((rows, N_OUT), SENTINEL, np.float32), True,
                    fill=SENTINEL)
        _lib.check(L().pk2_gemm_f32_rows(tb, rows, N_OUT, K, 1.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld, bp.ptr,
                                         iptr(dperm), mv, sp()))
        got = Cp.window()
        exact_equal(got[perm[:mv]], G.gemm_exact(A, Bm, 1.0, beta, C0, bias), "tb=%d beta=%g" % (tb, beta))
        assert (got[perm[mv:]] == np.float32(SENTINEL)).all() and Cp.outside_untouched(np.float32(SENTINEL))


@pytest.mark.parametrize("arith", ARITH)
def test_rows_slice_rule_of_the_mapped_products_exact(arith, gemm_arith, monkeypatch):
    """1030 valid rows of 1200, 1024 columns, K = 1024: 72 (dX) and 64 (dW) tiles of 128 x 128 with K >= 1024 -- the range in which
    the mapped products choose their own slice count (gemm_launch: rows_rule) -- exact on integer operands with the rule and
    with PK2_GEMM_ROWS_SLICES=0 (read once per process: whichever the process runs under)."""
    gemm_arith(arith)
    set_env(monkeypatch, {})
    T, B, lengths, N, K = 300, 4, (300, 280, 250, 200), 1024, 1024
    perm, mv, dperm = batch(T, B, lengths)
    rows = T * B
    A, Bm = G.exact_family("b", mv, N, K, seed=11)                # dX form: A [Mv, K] sparse, B [K, N] dense
    C0, bias = G.exact_extras(mv, N, seed=12, bias=True)
    Ap, Bp, bp = Placed(scatter(A, rows, perm, mv), True), Placed(Bm, True), Placed(bias[None, :], True)
    Cp = Placed(scatter(C0, rows, perm, mv, SENTINEL), True, fill=SENTINEL)
    _lib.check(L().pk2_gemm_f32_rows(0, rows, N, K, 1.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, 1.0, Cp.ptr, Cp.ld, bp.ptr, iptr(dperm), mv, sp()))
    got = Cp.window()
    exact_equal(got[perm[:mv]], G.gemm_exact(A, Bm, 1.0, 1.0, C0, bias), "dX")
    assert (got[perm[mv:]] == np.float32(SENTINEL)).all() and Cp.outside_untouched(np.float32(SENTINEL))
    At, Y = G.exact_family("b", N, N, mv, seed=13)                # dW form: A^T [M = 1024, Kv] sparse, Y [Kv, N] dense
    Aw = At.T.copy()
    W0, _ = G.exact_extras(N, N, seed=14, bias=False)
    cs0 = np.arange(N, dtype=np.float32) % 7 - 3
    Awp, Yp = Placed(scatter(Aw, rows, perm, mv), True), Placed(scatter(Y, rows, perm, mv), True)
    Wp, csp = Placed(W0, True, fill=SENTINEL), Placed(cs0[None, :], True, fill=SENTINEL)
    _lib.check(L().pk2_gemm_f32_tn_colsum_rows(N, N, rows, 1.0, Awp.ptr, Awp.ld, Yp.ptr, Yp.ld, 1.0, Wp.ptr, Wp.ld, csp.ptr, iptr(dperm), mv,
                                               sp()))
    exact_equal(Wp.window(), G.gemm_exact(At, Y, 1.0, 1.0, W0), "dW")
    exact_equal(csp.window(), Aw.astype(np.float64).sum(0)[None, :] + cs0, "colsum")
    assert Wp.outside_untouched(np.float32(SENTINEL)) and csp.outside_untouched(np.float32(SENTINEL))


# weight-gradient form: (T, B, lengths, M, N) -- the last one has Kv = 1800 >= 1536 on two tiles: the K-slice rule engages
WGRAD = [(T, B, ln, N_OUT, K_IN) for T, B, ln in BATCHES] + [(600, 4, (600, 500, 400, 300), N_OUT, 64)]


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("T,B,lengths,M,N", WGRAD)
@pytest.mark.parametrize("env", [{}, {"PK2_GEMM_TILES": "1"}, {"PK2_GEMM_SPLITK": "3"}])
def test_rows_weight_gradient_and_colsum_exact(T, B, lengths, M, N, env, arith, gemm_arith, monkeypatch):
    gemm_arith(arith)
    set_env(monkeypatch, env)
    perm, mv, dperm = batch(T, B, lengths)
    rows = T * B
    At, Bm = G.exact_family("b", M, N, mv, seed=rows)             # A^T [M, Kv] sparse {0, +-1, +-2}: exact column sums
    A = At.T.copy()
    for aligned, beta in ((True, 1.0), (False, 0.0)):
        C0, _ = G.exact_extras(M, N, seed=mv, bias=False)
        cs0 = np.arange(M, dtype=np.float32) % 7 - 3
        want_c = G.gemm_exact(At, Bm, 2.0, beta, C0)
        want_cs = A.astype(np.float64).sum(0)[None, :] + cs0
        Ap, Bp = Placed(scatter(A, rows, perm, mv), aligned), Placed(scatter(Bm, rows, perm, mv), aligned)
        for form in ("map", "pack"):
            Cp = Placed(C0 if beta != 0.0 else np.full(C0.shape, np.nan, np.float32), aligned, fill=SENTINEL)
            csp = Placed(cs0[None, :], aligned, fill=SENTINEL)
            if form == "map":
                _lib.check(L().pk2_gemm_f32_tn_colsum_rows(M, N, rows, 2.0, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld, beta, Cp.ptr, Cp.ld, csp.ptr,
                                                           iptr(dperm), mv, sp()))
            else:
                a_p = torch.full((mv, M), float("nan"), device="cuda")
                b_p = torch.full((mv, N), float("nan"), device="cuda")
                _lib.check(L().pk2_rows_pack(Ap.ptr, Ap.ld, M, iptr(dperm), mv, _lib.ptr(a_p), M, sp()))
                _lib.check(L().pk2_rows_pack(Bp.ptr, Bp.ld, N, iptr(dperm), mv, _lib.ptr(b_p), N, sp()))
                assert np.array_equal(a_p.cpu().numpy(), A) and np.array_equal(b_p.cpu().numpy(), Bm)
                _lib.check(L().pk2_gemm_f32_tn_colsum(M, N, mv, 2.0, _lib.ptr(a_p), M, _lib.ptr(b_p), N, beta, Cp.ptr, Cp.ld, csp.ptr,
                                                      sp()))
            exact_equal(Cp.window(), want_c, "%s C" % form)
            exact_equal(csp.window(), want_cs, "%s colsum" % form)
            assert Cp.outside_untouched(np.float32(SENTINEL)) and csp.outside_untouched(np.float32(SENTINEL))


@pytest.mark.parametrize("arith", ARITH)
def test_identity_map_gives_the_unmapped_bits(arith, gemm_arith, monkeypatch):
    gemm_arith(arith)
    set_env(monkeypatch, {})
    T, B = 7, 3
    rows = T * B
    perm, mv = row_map_host((T,) * B, T, B)
    assert mv == rows and np.array_equal(perm, np.arange(rows))
    dperm = torch.from_numpy(perm).cuda()
    A, Bm = G.random_case("normal", rows, N_OUT, K_IN, seed=5)
    a, bt, b = torch.from_numpy(A).cuda(), torch.from_numpy(Bm.T.copy()).cuda(), torch.from_numpy(Bm).cuda()
    for tb, bmat in ((1, bt), (0, b)):
        ref = torch.full((rows, N_OUT), float("nan"), device="cuda")
        _lib.check(L().pk2_gemm_f32(0, tb, rows, N_OUT, K_IN, 1.0, _lib.ptr(a), K_IN, _lib.ptr(bmat), bmat.shape[1], 0.0, _lib.ptr(ref),
                                    N_OUT, None, sp()))
        for rmap in (iptr(dperm), None):
            c = torch.full((rows, N_OUT), float("nan"), device="cuda")
            _lib.check(L().pk2_gemm_f32_rows(tb, rows, N_OUT, K_IN, 1.0, _lib.ptr(a), K_IN, _lib.ptr(bmat), bmat.shape[1], 0.0,
                                             _lib.ptr(c), N_OUT, None, rmap, rows if rmap is not None else 5, sp()))
            assert torch.equal(c.view(torch.int32), ref.view(torch.int32))
    # weight-gradient form: dW = A^T Y over all rows, colsum accumulated
    y = torch.from_numpy(G.random_case("normal", rows, 1, 8, seed=6)[0]).cuda()              # [rows, 8]
    outs = []
    for rmap, kv in ((None, 3), (iptr(dperm), rows), ("plain", 0)):
        c = torch.zeros(K_IN, 8, device="cuda")
        cs = torch.zeros(K_IN, device="cuda")
        if rmap == "plain":
            _lib.check(L().pk2_gemm_f32_tn_colsum(K_IN, 8, rows, 1.0, _lib.ptr(a), K_IN, _lib.ptr(y), 8, 1.0, _lib.ptr(c), 8, _lib.ptr(cs),
                                                  sp()))
        else:
            _lib.check(L().pk2_gemm_f32_tn_colsum_rows(K_IN, 8, rows, 1.0, _lib.ptr(a), K_IN, _lib.ptr(y), 8, 1.0, _lib.ptr(c), 8,
                                                       _lib.ptr(cs), rmap, kv, sp()))
        outs.append((c.cpu(), cs.cpu()))
    # (C: plain stores, the same bits.  The column sums are added with float atomics -- in LDS and in memory -- in arrival
    # order: two calls of the SAME entry may differ in the last bits, so they are held to the f32 floor of a 21-term sum)
    for c, cs in outs[:2]:
        assert torch.equal(c.view(torch.int32), outs[2][0].view(torch.int32))
        assert float((cs - outs[2][1]).abs().max()) <= 21 * 2.0 ** -23 * float(a.abs().sum(0).max())
