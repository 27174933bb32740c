"""oracle/gemm_ref.py, the host reference of the pk2_gemm_f32 family: its fixtures and bounds must tell a correct kernel from a
subtly broken one, or a device test passing on them means nothing.  CPU only."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import gemm_ref as G

SHAPES = [(1, 1, 1), (3, 5, 17), (2, 65, 256), (65, 129, 1030), (5, 3, 4100)]


def test_split3_is_exact_and_round_to_nearest_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000), rng.standard_normal(1000) * 1e30, rng.standard_normal(1000) * 1e-20]).astype(np.float32)
    h, m, lo = G.split3(x)
    assert np.array_equal(h.astype(np.float64) + m + lo, x.astype(np.float64))
    for p in (h, m, lo):
        assert not (p.view(np.uint32) & 0xFFFF).any()
    # ties to even: 1 + 2^-8 (halfway between 1 and 1 + 2^-7) -> 1; 1 + 3 * 2^-8 -> 1 + 2^-6
    assert G.bf16_rne(np.float32([1 + 2 ** -8, 1 + 3 * 2 ** -8])).tolist() == [1.0, 1 + 2 ** -6]
    assert np.array_equal(torch.from_numpy(x).to(torch.bfloat16).float().numpy(), h)


@pytest.mark.parametrize("fam", "abc")
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_families_are_exact_everywhere_and_catch_every_mutation_they_should(fam, M, N, K):
    A, B = G.exact_family(fam, M, N, K, seed=M + K)
    want = G.gemm_exact(A, B)
    assert np.array_equal(want.astype(np.float32), want)
    assert np.array_equal((torch.from_numpy(A) @ torch.from_numpy(B)).numpy(), want)
    assert np.array_equal(G.x3_product(A, B), want)
    assert np.array_equal(G.fmaf_chain(A, B), want) and np.array_equal(G.serial_f32(A, B), want)
    ah, am, al = G.split3(A)
    bh, bm, bl = G.split3(B)
    # the planes each family exercises
    if fam == "a":
        assert (al != 0).all() and (am != 0).all() and not bm.any() and not bl.any()
    if fam == "b":
        assert (bl != 0).all() and (bm != 0).all() and not am.any() and not al.any()
    if fam == "c":
        assert (am != 0).all() and np.array_equal(bm != 0, B != 0) and not al.any() and not bl.any()
    caught = {m for m in G.MUTATIONS if not np.array_equal(G.x3_product(A, B, m), want)}
    need = {"a": {"drop_lh", "zero_lo_a", "hi_only"}, "b": {"drop_hl", "zero_lo_b", "hi_only"}, "c": {"drop_mm", "hi_only"}}[fam]
    assert caught == need


def test_every_mutation_is_caught_by_some_family():
    caught = set()
    for fam in "abc":
        A, B = G.exact_family(fam, 64, 64, 300, seed=3)
        want = G.gemm_exact(A, B)
        caught |= {m for m in G.MUTATIONS if not np.array_equal(G.x3_product(A, B, m), want)}
    assert caught == set(G.MUTATIONS)


def test_exact_family_with_power_of_two_row_and_column_scales():
    rng = np.random.default_rng(1)
    M, N, K = 33, 40, 200
    re, ce = rng.integers(-30, 31, size=M), rng.integers(-30, 31, size=N)
    for fam in "abc":
        A, B = G.exact_family(fam, M, N, K, seed=5, row_exp=re, col_exp=ce)
        C0, bias = G.exact_extras(M, N, seed=5, row_exp=re, col_exp=ce)
        assert bias is None
        want = G.gemm_exact(A, B, 2.0, 0.5, C0)
        assert np.array_equal(want.astype(np.float32), want)
        got = 2.0 * G.x3_product(A, B) + np.float32(0.5) * C0
        assert np.array_equal(got, want)
        assert not np.array_equal(G.x3_product(A, B, "hi_only"), G.gemm_exact(A, B))


def test_k_positions_cover_the_edges():
    rng = np.random.default_rng(0)
    for K in (1, 3, 17, 256, 1030, 4100):
        ks = G.k_positions(K, rng, 16)
        assert len(set(ks.tolist())) == len(ks) == min(16, K)
        assert 0 in ks and K - 1 in ks and ks.max() < K


def test_fmaf_is_correctly_rounded():
    rng = np.random.default_rng(2)
    a = rng.standard_normal(3000).astype(np.float32)
    b = rng.standard_normal(3000).astype(np.float32)
    c = rng.standard_normal(3000).astype(np.float32)
    # a second set whose exact a b + c lies at or next to a float32 midpoint: c = -(a b rounded to float32) + a half ulp of 1
    c2 = (-(a.astype(np.float64) * b) + np.float32(1.0) + 2.0 ** -24).astype(np.float32)
    for cc in (c, c2):
        got = G.fmaf(a, b, cc)
        for i in range(0, 3000, 3):
            ex = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(cc[i]))
            f = np.float32(float(ex))
            cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
            best = min(cands, key=lambda x: (abs(Fraction(float(x)) - ex), int(np.float32(x).view(np.uint32)) & 1))
            assert got[i] == best, (i, a[i], b[i], cc[i])
    # the fmaf chain rounds once per k, the serial one twice: they differ
    A, B = G.random_case("normal", 16, 16, 64, seed=1)
    assert not np.array_equal(G.fmaf_chain(A, B), G.serial_f32(A, B))


@pytest.mark.parametrize("kind,K", [("act_w", 64), ("act_w", 256), ("act_w", 1024), ("normal", 64), ("normal", 1024),
                                    ("wgrad", 1024)])
def test_statistical_bound_accepts_correct_arithmetic_and_rejects_every_mutation(kind, K):
    A, B = G.random_case(kind, 128, 128, K, seed=K)
    x3r, x3m = G.STAT_BOUND["bf16x3"]
    f32r, f32m = G.STAT_BOUND["f32"]
    rms, mx = G.err_units(G.x3_product(A, B), A, B)
    assert rms * 2 <= x3r and mx * 2 <= x3m, (rms, mx)
    for got in (A @ B, G.fmaf_chain(A, B)):
        rms, mx = G.err_units(got, A, B)
        assert rms * 2 <= f32r and mx * 2 <= f32m, (rms, mx)
    for m in G.MUTATIONS:
        rms, mx = G.err_units(G.x3_product(A, B, m), A, B)
        assert rms > x3r and rms > f32r, (m, rms)
        if m == "hi_only":
            assert mx > x3m and mx > f32m, (m, mx)


def test_err_units():
    A = np.float32([[1.0, -2.0]])
    B = np.float32([[3.0], [1.0]])
    assert G.err_units(np.float32([[1.0]]), A, B) == (0.0, 0.0)
    # unit = 2 |1 * 3| + 2 |-2 * 1| + |0.5 * 4| + |1| = 13
    rms, mx = G.err_units(np.float32([[2 * 1 + 0.5 * 4 + 1 + 1.3]]), A, B, 2.0, 0.5, np.float32([[4.0]]), np.float32([1.0]))
    assert abs(mx - 0.1) < 1e-7 and abs(rms - 0.1) < 1e-7
    assert G.err_units(np.float32([[1.0]]), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32))[1] == np.inf
