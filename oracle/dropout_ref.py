"""The counter-based dropout mask of include/pk2hip.h (pk2_dropout_f32; pk2_attention_fwd / _bwd index the same mask like a
[B*H][T][T] matrix), numpy only.

Written from the definition in the header and csrc/dropout.hip: the mask is a pure function of (seed, element index i),

    z = seed * 0xD1342543DE82EF95 + i                       (uint64, wrapping)
    z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31
    keep element i  <=>  uint32(z >> 32) < uint32(min(4294967295, keep * 2^32)),      keep = 1 - double(float32(p))
    y = x * float32(1 / keep) where kept, 0 elsewhere
"""
import numpy as np

_U = np.uint64


def keep_mask(seed, n, p):
    """(mask, scale): bool [n], True where element i is kept, and the float32 factor kept elements are multiplied by."""
    keep = 1.0 - float(np.float32(p))
    assert 0.0 < keep <= 1.0, p
    threshold = np.uint32(int(min(4294967295.0, keep * 4294967296.0)))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=_U) + np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], _U) * _U(0xD1342543DE82EF95)
        z += _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        z ^= z >> _U(31)
    return (z >> _U(32)).astype(np.uint32) < threshold, np.float32(1.0 / keep)
