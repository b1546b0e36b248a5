"""GPU: pgx_dft_c2c -- the arbitrary-length float64 DFT of csrc/pgx_spectral.hip -- against numpy.fft in float64.

Bound (set before any device run): max |X_dev - X_numpy| <= 8 * 2^-52 * max(1, log2 M) * max |X_numpy|, M the power-of-two
transform behind the length (N itself on the direct path, Bluestein's 2^ceil(log2(2N-1)) otherwise).  A power-of-two
FFT's rounding error grows like eps * log2 M; Bluestein chains three of them plus a chirp good to an ulp.  A numpy model
of exactly this algorithm stays below 0.3 * eps * log2 M at the long lengths (tests/test_tralfam_host.py recomputes
that at test time); the factor 8 is room for FMA contraction, the radix order and the device sincos, and sits six
orders of magnitude below a single-precision mistake.  Every length runs once."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LENGTHS = (1, 2, 3, 7, 128, 1000, 4096, 65_536, 4097, 16_964, 105_164, 99_991, 132_300, 156_168, 1_048_577,
           2 ** 21 - 1, 2 ** 21)


def _fft_points(n: int) -> int:
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def _bound(n: int, ref: np.ndarray) -> float:
    return 8.0 * EPS * max(1.0, np.log2(_fft_points(n))) * float(np.max(np.abs(ref)))


def _signal(n: int) -> np.ndarray:
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    x[1] *= np.exp(-np.arange(n) / max(1.0, n / 8.0))          # a decaying row
    x[2] = np.exp(2j * np.pi * 0.123456 * np.arange(n)) + 0.5   # a tone off the bin grid plus DC
    return x


@pytest.mark.parametrize("n", LENGTHS)
def test_dft_matches_numpy(n):
    from pygmu2_amd import spectral
    x = _signal(n)
    fwd_ref = np.fft.fft(x, axis=-1)
    inv_ref = np.fft.ifft(x, axis=-1)
    for batch in (1, 2, 3):
        fwd = spectral.dft(x[:batch])
        err = float(np.max(np.abs(fwd - fwd_ref[:batch])))
        bound = _bound(n, fwd_ref[:batch])
        print(f"n={n} batch={batch} forward err={err:.3e} bound={bound:.3e}")
        assert err <= bound, f"forward n={n} batch={batch}: {err:.3e} > {bound:.3e}"
        inv = spectral.dft(x[:batch], inverse=True)
        err = float(np.max(np.abs(inv - inv_ref[:batch])))
        bound = _bound(n, inv_ref[:batch])
        print(f"n={n} batch={batch} inverse err={err:.3e} bound={bound:.3e}")
        assert err <= bound, f"inverse n={n} batch={batch}: {err:.3e} > {bound:.3e}"
    back = spectral.dft(spectral.dft(x), inverse=True)
    # two transforms: the forward error (relative to max |X|) comes back through an inverse that scales by 1/n
    bound = 2.0 * 8.0 * EPS * max(1.0, np.log2(_fft_points(n))) * float(np.max(np.abs(x))) * np.sqrt(n)
    err = float(np.max(np.abs(back - x)))
    print(f"n={n} round trip err={err:.3e} bound={bound:.3e}")
    assert err <= bound


def test_one_dimensional_input_and_plan_reuse():
    from pygmu2_amd import spectral
    x = np.arange(12, dtype=np.float64) + 0j
    assert spectral.dft(x).shape == (12,)
    assert spectral.plan_for(12) is spectral.plan_for(12)
    np.testing.assert_allclose(spectral.dft(x), np.fft.fft(x), atol=8 * EPS * 4 * 66.0)


def test_length_past_the_limit_is_a_value_error():
    from pygmu2_amd import spectral
    from pygmu2_amd._kernels import lib
    limit = spectral.max_length()
    assert limit == 2 ** 21
    with pytest.raises(ValueError, match=str(limit)):
        spectral.DftPlan(limit + 1)
    # the entry point itself refuses too (PGX_ERR_INVALID)
    assert lib().pgx_dft_plan(1, limit + 1) == -1
    assert lib().pgx_dft_c2c(1, 1, limit + 1, 1, 0, 1, 1) == -1
