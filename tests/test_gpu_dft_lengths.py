"""GPU: pgx_dft_c2c at every size class and call form of csrc/pgx_spectral.hip, in float64.

tests/test_gpu_dft.py runs seventeen lengths, in place, through spectral.dft.  This module runs what those leave out:
every length 1..1100 (every LDS tile length 0..11 directly and through Bluestein, the first two-pass Bluestein), the
whole power-of-two ladder 2^0..2^21 (every four-step split), the shortest and the longest N behind every Bluestein
M = 2^5..2^22, out-of-place calls, batches that do not fill, exactly fill and just overflow a tile, the batch limit, the
plan's own contents, and TralfamPE at the size classes its fixtures do not hold.  tests/test_dft_reference_host.py
proves the coverage from the length lists (tests/dft_reference.py) and checks the references on the CPU.

Bounds, none set from a device run: every transform tralfam_oracle.dft_bound = 8 * 2^-52 * max(1, log2 M) * max |ref|
(the bound of tests/test_gpu_dft.py); a chirp component 4e-16 absolute (the bound tests/test_gpu_math.py holds the same
polynomials to); TralfamPE fixture_harness.PEAK_BOUND.  References: the O(N^2) long-double DFT up to N = 256, numpy.fft
above, and two closed forms (impulse, tone on the bin grid) at the longest lengths.  Every comparison prints
"DFT_LEN <class> ... err= bound= ratio=" before it asserts; profiles/dft_lengths.md holds the worst ratio per class."""

import numpy as np
import pytest

import dft_reference as R
import fixture_harness as H
import tralfam_oracle as T
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

PGX_ERR_INVALID = -1
TILE = 1 << R.TILE_LOG2


def _rows(n: int, batch: int, salt: int = 0) -> np.ndarray:
    """`batch` distinct random complex rows of n points."""
    rng = np.random.default_rng([n, batch, salt])
    return rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))


def _class_tag(n: int) -> str:
    c = R.size_classes(n)
    route = "direct" if c["bluestein"] is None else f"bluestein-M2^{c['bluestein']}"
    return route + (f" tile-l{c['tile']}" if c["split"] is None else f" split-{c['split'][0]}/{c['split'][1]}")


def _held(what: str, n: int, got: np.ndarray, ref: np.ndarray, failures=None):
    """One comparison: printed, then asserted (or collected into `failures`, so that a sweep reports every miss)."""
    err = R.max_err(got, ref)
    bound = T.dft_bound(n, np.asarray(ref).astype(np.complex128))
    print(f"DFT_LEN {_class_tag(n)} {what} n={n} err={err:.3e} bound={bound:.3e} ratio={err / bound:.3f}")
    ok = np.all(np.isfinite(np.asarray(got).view(np.float64))) and err <= bound
    if failures is None:
        assert ok, f"{what} n={n}: {err:.3e} > {bound:.3e}"
    elif not ok:
        failures.append(f"{what} n={n}: {err:.3e} > {bound:.3e}")
    return err / bound


def _both_directions(n: int, batch: int, reference, failures=None, what=""):
    from pygmu2_amd import spectral
    x = _rows(n, batch)
    for inverse in (False, True):
        got = spectral.dft(x, inverse=inverse)
        _held(f"{what}batch={batch} {'inverse' if inverse else 'forward'}", n, got, reference(x, inverse),
              failures=failures)


def _numpy_reference(x, inverse):
    return np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1)


# ------------------------------------------------------------------------------------------------- 1. every small length
@pytest.mark.parametrize("lengths", R.chunks(R.LONGDOUBLE_LENGTHS), ids=lambda c: f"{c[0]}-{c[-1]}")
def test_small_lengths_against_the_longdouble_dft(lengths):
    failures = []
    for n in lengths:
        _both_directions(n, 2, R.dft_longdouble, failures, "vs-longdouble ")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("lengths", R.chunks(R.NUMPY_LENGTHS), ids=lambda c: f"{c[0]}-{c[-1]}")
def test_small_lengths_against_numpy(lengths):
    failures = []
    for n in lengths:
        _both_directions(n, 2, _numpy_reference, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------- 2. the ladders
def _closed_forms(n: int):
    from pygmu2_amd import spectral
    _held("impulse", n, spectral.dft(R.impulse(n)), R.impulse_spectrum(n))          # max |ref| = 1
    _held("tone", n, spectral.dft(R.tone(n)), R.tone_spectrum(n))                   # max |ref| = n


@pytest.mark.parametrize("m", R.DIRECT_LOG2)
def test_power_of_two_ladder(m):
    n = 1 << m
    _both_directions(n, 2, _numpy_reference)
    if n in R.CLOSED_FORM_DIRECT:
        _closed_forms(n)


@pytest.mark.parametrize("m", R.BLUESTEIN_LOG2)
def test_bluestein_ends_of_every_m(m):
    for n in R.bluestein_pair(m):
        assert T.fft_points(n) == 1 << m
        _both_directions(n, 2 if m <= 19 else 1, _numpy_reference)
        if n in R.CLOSED_FORM_BLUESTEIN:
            _closed_forms(n)


# ------------------------------------------------------------------------------------------------- 3. call forms, C ABI
class _Transform:
    """pgx_dft_plan + pgx_dft_workspace_bytes + pgx_dft_c2c over device buffers of this object's own."""

    def __init__(self, n: int, batch: int):
        from pygmu2_amd._kernels import DeviceBuffer, check, lib
        self.n, self.batch, self.lib, self.check, self.Buffer = n, batch, lib(), check, DeviceBuffer
        self.plan = DeviceBuffer((self.lib.pgx_dft_plan_bytes(n),), np.uint8)
        check(self.lib.pgx_dft_plan(self.plan.ptr, n), "pgx_dft_plan")
        need = self.lib.pgx_dft_workspace_bytes(n, batch)
        assert need > 0
        self.work = DeviceBuffer((need,), np.uint8)

    def run(self, x: np.ndarray, inverse: bool, in_place: bool):
        """-> (the result, the input buffer read back afterwards)."""
        assert x.shape == (self.batch, self.n) and x.dtype == np.complex128
        src = self.Buffer.from_host(x.view(np.float64))
        dst = src if in_place else self.Buffer(src.shape, np.float64)
        self.check(self.lib.pgx_dft_c2c(dst.ptr, src.ptr, self.n, self.batch, int(inverse), self.plan.ptr,
                                        self.work.ptr), "pgx_dft_c2c")
        return dst.to_host().view(np.complex128), src.to_host().view(np.complex128)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def _rows_held(what: str, n: int, got: np.ndarray, ref: np.ndarray, show=()):
    """Every row against its own reference row and its own bound: a row that took its neighbour's place is far out."""
    err = np.max(np.abs(got - ref), axis=1)
    bound = T.dft_bound(n, np.ones(1)) * np.max(np.abs(ref), axis=1)          # dft_bound of each row
    assert np.all(np.isfinite(got.view(np.float64))), f"{what} n={n}: not finite"
    worst = int(np.argmax(err / bound))
    for row in sorted(set(show) | {worst}):
        print(f"DFT_LEN {_class_tag(n)} {what} rows={got.shape[0]} row={row} n={n} err={err[row]:.3e} "
              f"bound={bound[row]:.3e} ratio={err[row] / bound[row]:.3f}")
    bad = np.flatnonzero(err > bound)
    assert not bad.size, f"{what} n={n}: rows {bad[:8].tolist()} of {got.shape[0]} miss the bound"


@pytest.mark.parametrize("n", (4, 32, 1000, 4096, 8192, 12_001))
def test_out_of_place_equals_in_place_and_keeps_its_input(n):
    x = _rows(n, 2, salt=3)
    with guarded():
        t = _Transform(n, 2)
        for inverse in (False, True):
            out, after = t.run(x, inverse, in_place=False)
            _held(f"out-of-place {'inverse' if inverse else 'forward'}", n, out, _numpy_reference(x, inverse))
            assert np.array_equal(_bits(after), _bits(x)), f"n={n}: the input of an out-of-place call changed"
            same, _ = t.run(x, inverse, in_place=True)
            assert np.array_equal(_bits(out), _bits(same)), f"n={n}: out of place differs from in place"


def _tile_fill_cases():
    out = []
    for m in (0, 2, 5, 11):
        per_tile = TILE >> m
        for batch in (per_tile - 1, per_tile, per_tile + 1, 2 * per_tile + 1):
            if batch >= 1:
                out.append((m, batch))
    return out


@pytest.mark.parametrize("m,batch", _tile_fill_cases())
def test_batches_around_a_full_tile(m, batch):
    n = 1 << m
    x = _rows(n, batch, salt=4)
    with guarded():
        t = _Transform(n, batch)
        for inverse in (False, True):
            out, _ = t.run(x, inverse, in_place=False)
            _rows_held(f"tile-fill {'inverse' if inverse else 'forward'}", n, out, _numpy_reference(x, inverse))


@pytest.mark.parametrize("n", (4096, 3000))
def test_two_pass_batch_of_five(n):
    x = _rows(n, 5, salt=5)
    with guarded():
        t = _Transform(n, 5)
        for inverse in (False, True):
            out, _ = t.run(x, inverse, in_place=False)
            _rows_held(f"two-pass-batch {'inverse' if inverse else 'forward'}", n, out, _numpy_reference(x, inverse))


@pytest.mark.parametrize("n", (1, 3))
def test_largest_batch(n):
    batch = 65_535
    x = _rows(n, batch, salt=6)
    with guarded():
        t = _Transform(n, batch)
        for inverse in (False, True):
            out, _ = t.run(x, inverse, in_place=False)
            _rows_held(f"batch-limit {'inverse' if inverse else 'forward'}", n, out, _numpy_reference(x, inverse),
                       show=(0, 1, 2047, 2048, 65_534))


@pytest.mark.parametrize("n", (1, 3))
def test_batch_past_the_limit_is_refused_without_a_launch(n):
    from pygmu2_amd._kernels import DeviceBuffer, lib
    batch = 65_536
    with guarded():
        t = _Transform(n, batch - 1)
        assert lib().pgx_dft_workspace_bytes(n, batch) == 0
        src = DeviceBuffer.from_host(_rows(n, batch, salt=7).view(np.float64))
        dst = DeviceBuffer(src.shape, np.float64)
        before = dst.to_host()
        assert lib().pgx_dft_c2c(dst.ptr, src.ptr, n, batch, 0, t.plan.ptr, t.work.ptr) == PGX_ERR_INVALID
        assert lib().pgx_dft_c2c(src.ptr, src.ptr, n, batch, 1, t.plan.ptr, t.work.ptr) == PGX_ERR_INVALID
        assert np.array_equal(_bits(dst.to_host()), _bits(before)), "a refused call wrote its output"


# ------------------------------------------------------------------------------------------------- 4. the plan itself
@pytest.mark.parametrize("n", (3, 12, 1000, 4097, 99_991))
def test_plan_holds_the_chirp_and_its_spectrum(n):
    """Layout (include/pygmu_hip.h): chirp[n] | spectrum[M] | scratch."""
    points = T.fft_points(n)
    with guarded():
        t = _Transform(n, 1)
        plan = t.plan.to_host()
    assert plan.nbytes >= (n + points) * 16
    held = plan[:(n + points) * 16].view(np.complex128)
    chirp, spectrum = held[:n], held[n:]
    want = R.chirp_longdouble(n)
    err_re = float(np.max(np.abs(chirp.real.astype(R.LD) - want.real)))
    err_im = float(np.max(np.abs(chirp.imag.astype(R.LD) - want.imag)))
    print(f"DFT_LEN plan chirp n={n} err_re={err_re:.3e} err_im={err_im:.3e} bound=4.000e-16 "
          f"ratio={max(err_re, err_im) / 4e-16:.3f}")
    assert err_re <= 4e-16 and err_im <= 4e-16, f"chirp n={n}: {err_re:.3e}, {err_im:.3e} > 4e-16"
    _held("plan spectrum", n, spectrum, np.fft.fft(R.wrapped_chirp(n)))


# ------------------------------------------------------------------------------------------------- 5. TralfamPE
@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("n", (4, 32, 64, 8192, 32_768, 5000))
def test_tralfam_at_the_new_size_classes(n, channels):
    import pygmu2_amd as pg
    pg.set_sample_rate(48000)
    x = np.stack([T.hashed_noise(n, 0x9E3779B9 * (c + 1) & 0xFFFFFFFF) for c in range(channels)], axis=1)
    seed = 1000 * n + channels
    got = np.array(pg.TralfamPE(pg.ArrayPE(x), seed=seed, normalize_peak=None).render(0, n).data, dtype=np.float32)
    want = T.mogrify(x, seed, None)
    H.assert_peak(f"tralfam {_class_tag(n)} n={n} channels={channels}", got, want, H.PEAK_BOUND, "DFT_LEN")
