"""CPU: the references of tests/test_gpu_dft_lengths.py, checked before anything on a device is held to them, and the
proof that the lengths it runs reach every size class of pgx_dft_c2c.

The long-double DFT by the definition (tests/dft_reference.py) and numpy.fft agree within a tenth of the device's bound;
the closed forms (impulse, tone on the bin grid) hold for numpy.fft within the bound; the numpy model of the device's
route, tralfam_oracle.bluestein_dft, meets the bound against the long-double DFT; and the length lists, read with the
kernel's own routing rule, cover every LDS tile length 0..11 directly and through Bluestein, every four-step split
for m = 12..22 and every Bluestein M = 2^3..2^22."""

import numpy as np
import pytest

import dft_reference as R
import tralfam_oracle as T


def _rows(n: int, batch: int = 2) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps <= 2 ** -63
    # 2*pi itself carries the extra bits: its float64 rounding differs from it by less than half a float64 ulp, not 0
    assert 0 < abs(float(R.TWO_PI - np.longdouble(2 * np.pi))) < 2 ** -51


@pytest.mark.parametrize("n", tuple(range(1, 65)) + (255,))
def test_longdouble_dft_agrees_with_numpy(n):
    x = _rows(n)
    for inverse in (False, True):
        ref = R.dft_longdouble(x, inverse)
        got = np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1)
        err, bound = R.max_err(got, ref), T.dft_bound(n, ref.astype(np.complex128))
        assert err <= 0.1 * bound, f"n={n} inverse={inverse}: {err:.3e} > 0.1 * {bound:.3e}"


@pytest.mark.parametrize("n", tuple(range(3, 65)))
def test_bluestein_model_meets_the_bound_against_longdouble(n):
    x = _rows(n, 1)[0]
    for inverse in (False, True):
        ref = R.dft_longdouble(x, inverse)
        err, bound = R.max_err(T.bluestein_dft(x, inverse), ref), T.dft_bound(n, ref.astype(np.complex128))
        assert err <= bound, f"n={n} inverse={inverse}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("n", (1 << 20, (1 << 20) - 1, (1 << 19) + 1, 12, 7))
def test_closed_forms_hold_for_numpy(n):
    want = R.impulse_spectrum(n)
    assert np.max(np.abs(want)) == pytest.approx(1.0, abs=1e-15)
    err, bound = R.max_err(np.fft.fft(R.impulse(n)), want), T.dft_bound(n, want)
    assert err <= bound, f"impulse n={n}: {err:.3e} > {bound:.3e}"
    want = R.tone_spectrum(n)
    assert float(np.max(np.abs(want))) == n and np.count_nonzero(want) == 1
    err, bound = R.max_err(np.fft.fft(R.tone(n)), want), T.dft_bound(n, want)
    assert err <= bound, f"tone n={n}: {err:.3e} > {bound:.3e}"


def test_closed_forms_against_the_definition():
    for n in (7, 12, 64):
        assert R.max_err(R.impulse_spectrum(n), R.dft_longdouble(R.impulse(n))) <= 2 ** -52
        assert R.max_err(R.tone_spectrum(n), R.dft_longdouble(R.tone(n))) <= n * 2 ** -52


def test_chirp_reduces_its_phase_in_integers():
    n = 2 ** 21 - 1
    k = np.array([n - 1, n - 2, 1_500_000])
    b = R.chirp_longdouble(n)[k]
    for v, got in zip(k, b):
        r = int(v) ** 2 % (2 * n)                       # Python integers: exact
        a = R.TWO_PI * np.longdouble(r) / np.longdouble(2 * n)
        assert got.real == np.cos(a) and got.imag == np.sin(a)
    w =R.wrapped_chirp(12)
    assert w.shape == (32,) and w[0] == 1.0 and not np.any(w[12:21]) and np.array_equal(w[21:], w[1:12][::-1])


def test_bluestein_pairs_are_the_ends_of_what_m_serves():
    for m in R.BLUESTEIN_LOG2:
        lo, hi = R.bluestein_pair(m)
        for n in (lo, hi):
            assert n & (n - 1), n
            assert T.fft_points(n) == 1 << m, (m, n)
        assert T.fft_points(lo - 1) < 1 << m and T.fft_points(hi + 2) > 1 << m
    assert max(R.LADDER_LENGTHS) <= 2 ** 21
    assert R.CLOSED_FORM_DIRECT == (2 ** 19, 2 ** 20, 2 ** 21)
    assert R.CLOSED_FORM_BLUESTEIN == (2 ** 20 - 1, 2 ** 20 + 1, 2 ** 21 - 1)


def test_length_lists_cover_every_size_class():
    small = R.LONGDOUBLE_LENGTHS + R.NUMPY_LENGTHS
    assert small == tuple(range(1, 1101))
    assert [len(c) for c in R.chunks(R.LONGDOUBLE_LENGTHS)] == [100, 100, 56]
    assert sum(len(c) for c in R.chunks(R.NUMPY_LENGTHS)) == len(R.NUMPY_LENGTHS)
    classes = [R.size_classes(n) for n in small + R.LADDER_LENGTHS]
    tiles = set(range(R.TILE_LOG2 + 1))
    direct = {c["tile"] for c in classes if c["bluestein"] is None and c["tile"] is not None}
    assert direct == tiles, f"LDS tile lengths never run directly: {sorted(tiles - direct)}"
    through = {c["tile"] for c in classes if c["bluestein"] is not None and c["tile"] is not None}
    assert through == set(range(3, R.TILE_LOG2 + 1)), sorted(through)      # M = 8 is the smallest Bluestein serves
    splits = {m: (m // 2, m - m // 2) for m in range(12, 23)}
    got = {c["split"] for c in classes if c["split"] is not None}
    assert got == set(splits.values()), f"four-step splits never run: {sorted(set(splits.values()) - got)}"
    direct_splits = {c["split"] for c in classes if c["split"] is not None and c["bluestein"] is None}
    assert direct_splits == {splits[m] for m in range(12, 22)}             # 2^22 points: Bluestein's M alone
    ms = {c["bluestein"] for c in classes if c["bluestein"] is not None}
    assert ms == set(range(3, 23)), f"Bluestein M never run: {sorted(set(range(3, 23)) - ms)}"
    # the small lengths alone reach every tile length both ways, and the first two-pass Bluestein
    small_classes = [R.size_classes(n) for n in small]
    assert {c["tile"] for c in small_classes if c["bluestein"] is None} - {None} == set(range(11))
    assert {c["bluestein"] for c in small_classes} - {None} == set(range(3, 13))
