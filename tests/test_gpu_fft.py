"""The hand-written inverse real FFT (csrc/fft.hip, pk2_irfft_pow2_f32) against numpy.fft.irfft in float64: the smallest
length, the largest that one workgroup transforms in LDS (n = 8192), the smallest that takes the four-step form
(n = 16384), and n = 2^18 (the isotropic noise of a 10 s utterance); 3 rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# The rule of DESIGN.md 7.4: numpy's own irfft in float32 (numpy 2 keeps complex64 through np.fft) against float64 on the
# inputs below gave 8.8e-8 (n = 32), 1.32e-7 (8192), 1.48e-7 (16384), 1.69e-7 (2^18) relative to max|want|; 4 x the largest.
IRFFT_TOL = 4 * 1.69e-7
SIZES = [32, 8192, 16384, 1 << 18]


def _spectrum(n, rows=3):
    rs = np.random.RandomState(n)
    return (rs.standard_normal((rows, n // 2 + 1)) + 1j * rs.standard_normal((rows, n // 2 + 1))).astype(np.complex64)


@pytest.mark.parametrize("n", SIZES)
def test_gpu_irfft_matches_numpy(n):
    import torch
    from pykaldi2_amd import simulation
    X = _spectrum(n)                   # DC and Nyquist carry imaginary parts: numpy ignores them, so does the kernel
    d_X = torch.from_numpy(X).cuda()
    got = simulation.irfft_pow2(d_X)
    want = np.fft.irfft(X.astype(np.complex128), n, axis=1)
    assert got.shape == (3, n) and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print("irfft n = %d rel err %.3e bound %.3e" % (n, err, IRFFT_TOL))
    assert err <= IRFFT_TOL
    assert np.array_equal(d_X.cpu().numpy(), X)                      # the input is left alone
    assert torch.equal(got, simulation.irfft_pow2(d_X))              # and the result is reproducible (cached twiddles)


def test_gpu_irfft_of_a_pure_tone():
    """Bin 5 of n = 16384 is the cosine of 5 periods, amplitude 2 / n per unit: the index arithmetic of the four-step form."""
    import torch
    from pykaldi2_amd import simulation
    n = 16384
    X = torch.zeros(1, n // 2 + 1, dtype=torch.complex64, device="cuda")
    X[0, 5] = n / 2
    got = simulation.irfft_pow2(X).cpu().numpy()[0]
    assert np.abs(got - np.cos(2 * np.pi * 5 * np.arange(n) / n)).max() < 1e-5


def test_gpu_irfft_argument_errors():
    import torch
    from pykaldi2_amd import _lib, simulation
    with pytest.raises(_lib.Pk2Error):
        simulation.irfft_pow2(torch.zeros(2, 49, dtype=torch.complex64, device="cuda"))          # n = 96
    with pytest.raises(_lib.Pk2Error):
        simulation.irfft_pow2(torch.zeros(2, 9, dtype=torch.complex64, device="cuda"))           # n = 16 < 2^5
    with pytest.raises(ValueError):
        simulation.irfft_pow2(torch.zeros(2, 17, 2, device="cuda"))                              # not complex64
    with pytest.raises(ValueError):
        simulation.irfft_pow2(torch.zeros(17, dtype=torch.complex64, device="cuda"))             # not (rows, bins)
