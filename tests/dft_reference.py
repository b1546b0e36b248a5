"""References for the float64 DFT tests that do not come from an FFT, and the length lists those tests run.

(a) `dft_longdouble`: the O(N^2) definition.  The twiddle index (j*k) mod N is reduced in int64 first, so the angle
    2*pi*r/N is formed from an exact r < N; cos, sin and the sums are numpy.longdouble (x87 extended, eps 2^-63).  Its
    own error is a few 2^-64 * sqrt(N) * max|x|, three orders of magnitude below tralfam_oracle.dft_bound, and
    tests/test_dft_reference_host.py holds numpy.fft to a tenth of that bound against it.
(b) Closed forms: the spectrum of a unit impulse and a tone on the bin grid, from the same reduced index.
(c) `chirp_longdouble`: Bluestein's b_k = exp(i*pi*k^2/N) with (k*k) mod 2N reduced in int64.
(d) The lengths of tests/test_gpu_dft_lengths.py and `size_classes`, which restates how csrc/pgx_spectral.hip routes a
    length (an LDS tile of 2^l points, l <= 11; the four-step split l1 = m // 2, l2 = m - l1; Bluestein over
    M = 2^ceil(log2(2N-1))), so that the host test can prove from the lists which classes they reach.
"""

from __future__ import annotations

import numpy as np

import tralfam_oracle as T

LD = np.longdouble
CLD = np.clongdouble
# The hosts are x86-64.  A long double that is a plain double would make (a) no finer than what it judges.
assert np.finfo(LD).eps <= 2 ** -63, f"numpy.longdouble is not an extended type here (eps {np.finfo(LD).eps})"

TWO_PI = 8 * np.arctan(LD(1))
TILE_LOG2 = 11                                   # kTileLog2 of pgx_spectral.hip


# ------------------------------------------------------------------------------------------------- (a) - (c)
def cis_turns(r: np.ndarray, den: int) -> np.ndarray:
    """exp(2*pi*i * r / den) in long double for integers 0 <= r < den."""
    a = TWO_PI * np.asarray(r, dtype=np.int64).astype(LD) / LD(den)
    out = np.empty(a.shape, dtype=CLD)
    out.real = np.cos(a)
    out.imag = np.sin(a)
    return out


def dft_longdouble(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """numpy.fft.fft / ifft along the last axis of a (batch, n) or (n,) complex array by the definition -> clongdouble."""
    x = np.asarray(x)
    n = x.shape[-1]
    table = cis_turns(np.arange(n), n)                          # exp(+2*pi*i r/n)
    if not inverse:
        table = np.conj(table)
    j = np.arange(n, dtype=np.int64)
    w = table[(j[:, None] * j[None, :]) % n]                    # w[j, k], symmetric
    out = x.astype(CLD) @ w
    return out / LD(n) if inverse else out


def max_err(got: np.ndarray, ref: np.ndarray) -> float:
    """max |got - ref| with the difference taken in the reference's precision."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got).astype(ref.dtype) - ref))) if ref.size else 0.0


def impulse_index(n: int) -> int:
    return n // 3 + 1


def impulse(n: int) -> np.ndarray:
    x = np.zeros(n, dtype=np.complex128)
    x[impulse_index(n) % n] = 1.0
    return x


def impulse_spectrum(n: int) -> np.ndarray:
    """X[k] = exp(-2*pi*i * ((j0*k) mod n) / n) of `impulse(n)`, rounded from long double."""
    k = np.arange(n, dtype=np.int64)
    return np.conj(cis_turns(((impulse_index(n) % n) * k) % n, n)).astype(np.complex128)


def tone_bin(n: int) -> int:
    return n - 5


def tone(n: int) -> np.ndarray:
    """exp(+2*pi*i * ((k0*j) mod n) / n), k0 = n - 5, rounded from long double."""
    j = np.arange(n, dtype=np.int64)
    return cis_turns((tone_bin(n) * j) % n, n).astype(np.complex128)


def tone_spectrum(n: int) -> np.ndarray:
    x = np.zeros(n, dtype=np.complex128)
    x[tone_bin(n)] = n
    return x


def chirp_longdouble(n: int) -> np.ndarray:
    """b_k = exp(i*pi*k^2/n) = exp(2*pi*i * ((k*k) mod 2n) / 2n), k < n, in long double."""
    k = np.arange(n, dtype=np.int64)
    return cis_turns((k * k) % (2 * n), 2 * n)


def wrapped_chirp(n: int) -> np.ndarray:
    """The length-M kernel of Bluestein's convolution: b_j (j < n), b_(M-j) (j > M - n), 0 between."""
    m = T.fft_points(n)
    b = chirp_longdouble(n).astype(np.complex128)
    w = np.zeros(m, dtype=np.complex128)
    w[:n] = b
    w[m - n + 1:] = b[1:][::-1]
    return w


# ------------------------------------------------------------------------------------------------- (d) the lengths
LONGDOUBLE_LENGTHS = tuple(range(1, 257))        # against dft_longdouble
NUMPY_LENGTHS = tuple(range(257, 1101))          # against numpy.fft: up to Bluestein over M = 4096
DIRECT_LOG2 = tuple(range(0, 22))                # N = 2^m
BLUESTEIN_LOG2 = tuple(range(5, 23))             # M = 2^m behind the pair below


def bluestein_pair(m: int) -> tuple:
    """The shortest and the longest N that Bluestein serves with M = 2^m (m >= 3; neither a power of two for m >= 5)."""
    return (1 << m) // 4 + 1, (1 << m) // 2 - 1


LADDER_LENGTHS = tuple(1 << m for m in DIRECT_LOG2) + tuple(n for m in BLUESTEIN_LOG2 for n in bluestein_pair(m))
CLOSED_FORM_DIRECT = tuple(1 << m for m in DIRECT_LOG2[-3:])
CLOSED_FORM_BLUESTEIN = tuple(sorted(n for m in BLUESTEIN_LOG2 for n in bluestein_pair(m))[-3:])


def chunks(lengths, size: int = 100) -> list:
    return [tuple(lengths[i:i + size]) for i in range(0, len(lengths), size)]


def size_classes(n: int) -> dict:
    """How pgx_dft_c2c transforms length n: {"bluestein": log2 M or None, "tile": l or None (one launch),
    "split": (l1, l2) or None (two passes)}."""
    points = T.fft_points(n)
    m = points.bit_length() - 1
    two_pass = m > TILE_LOG2
    return {"bluestein": None if points == n else m,
            "tile": None if two_pass else m,
            "split": (m // 2, m - m // 2) if two_pass else None}
