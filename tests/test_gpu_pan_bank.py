"""GPU: the panned-voice kernels against pgx_pan itself, bit for bit.

pgx_pan_bank -- pgx_pan with the voice in the grid -- row by row against pgx_pan on that voice; pgx_pan_mix_batch against
pgx_pan per voice into [K][n][2] followed by pgx_mix_batch.  Both modes (linear, constant power), both forms: `gains` --
{lg, rg} per voice from pgx_pan_gains, scalar azimuths -- and `stream`, a row of azimuths per voice.  The scalar azimuths
hold both ends of the field, both zeros and values clipped on either side; the streams swing past +-90 degrees.  Every
device buffer lies between guard bands (tests/guarded_alloc.py); the rows are longer than their data, and the gaps, which
the guards do not see, hold a NaN pattern that must survive (in an output) and must not be read (in an input: a NaN in the
result shows it)."""

import numpy as np
import pytest

from guarded_alloc import guarded
from pygmu2_amd._kernels import DeviceBuffer, lib
from test_gpu_svf_bank import _padded, _pattern, _same

pytestmark = pytest.mark.gpu

PGX_OK, PGX_ERR_INVALID = 0, -1
AZIMUTHS = (-135.0, -90.0, -35.5, -0.0, 0.0, 45.0, 90.0, 90.0001, 200.0)
MODES = (0, 1)
FORMS = ("gains", "stream")
BATCHES = (1, 2, 31, 32, 33, 64, 65)          # the chunk edges of a 32-voice unroll
FRAMES = (1, 255, 256, 257, 1025)             # the workgroup edges and one grid-stride step (grid_for never caps these)
CHANNELS = (1, 2, 3, 8, 9)                    # row_mean changes form at 8
PADS = (7, 5, 3)                              # elements between the rows of: in, out, azimuth


def _scalars(batch):
    """Voice v's scalar azimuth: the list above, 3 degrees further for every round through it."""
    return np.array([AZIMUTHS[v % len(AZIMUTHS)] + 3.0 * (v // len(AZIMUTHS)) for v in range(batch)], dtype=np.float32)


def _streams(batch, n):
    """[batch][n] float32 azimuths that swing between -120 and 120 degrees, the scalar list planted at the front."""
    t = np.arange(n, dtype=np.float64)
    az = np.stack([120.0 * np.sin(0.05 * (v + 1) * t + 0.9 * v) for v in range(batch)]).astype(np.float32)
    planted = np.array(AZIMUTHS, dtype=np.float32)[:n]
    for v in range(batch):
        az[v, :len(planted)] = np.roll(planted, v)
    assert n < 64 or (az.max() > 90.0 and az.min() < -90.0)
    return az


def _inputs(batch, n, channels, seed):
    """[batch][n][channels] uniform(-1, 1); voice 0 holds an exact +0.0 and an exact -0.0 frame where there is room."""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, (batch, n, channels)).astype(np.float32)
    if n >= 4:
        x[0, n // 2, :] = np.float32(0.0)
        x[0, n // 3, :] = np.float32(-0.0)
    return x


def _pan(x, az, mode):
    """pgx_pan over one voice: az a number or (n,) float32 -> (n, 2)."""
    L = lib()
    n, channels = x.shape
    src, out = DeviceBuffer.from_host(x), DeviceBuffer((n, 2), np.float32)
    stream = DeviceBuffer.from_host(az) if isinstance(az, np.ndarray) else None
    rc = L.pgx_pan(out.ptr, src.ptr, n, channels, 0.0 if stream is not None else float(az),
                   stream.ptr if stream is not None else None, mode)
    assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host()


def _gains(scalars, mode):
    L = lib()
    az = DeviceBuffer.from_host(scalars)
    gains = DeviceBuffer((len(scalars), 2), np.float32)
    assert L.pgx_pan_gains(gains.ptr, az.ptr, len(scalars), mode) == PGX_OK, L.pgx_last_error()
    return gains


class _Args:
    """What both entries take behind `out`, uploaded: padded input rows, and gains or padded azimuth rows."""

    def __init__(self, x, form, mode):
        self.batch, self.n, self.channels = x.shape
        self.mode = mode
        self.in_stride, self.az_stride = self.n * self.channels + PADS[0], self.n + PADS[2]
        self.src = DeviceBuffer.from_host(_padded(x.reshape(self.batch, -1), self.in_stride, 11))
        self.scalars = _scalars(self.batch)
        self.streams = _streams(self.batch, self.n) if form == "stream" else None
        self.gains = _gains(self.scalars, mode) if form == "gains" else None
        self.az = DeviceBuffer.from_host(_padded(self.streams, self.az_stride, 23)) if form == "stream" else None

    def azimuth(self, v):
        return self.scalars[v] if self.streams is None else self.streams[v]

    def rows(self):
        return (self.src.ptr, self.in_stride, self.batch, self.n, self.channels,
                self.gains.ptr if self.gains else None, self.az.ptr if self.az else None, self.az_stride, self.mode)


# ------------------------------------------------------------------------------------------ 1. pgx_pan_gains
@pytest.mark.parametrize("mode", MODES)
def test_gains_are_what_pan_multiplies_by(mode):
    """pgx_pan of a source of ones gives {1 * lg, 1 * rg}: the pair pgx_pan_gains writes, bit for bit."""
    scalars = _scalars(300)                                       # (more than one workgroup of voices)
    with guarded():
        got = _gains(scalars, mode).to_host()
        ones = np.ones((1, 1), dtype=np.float32)
        for v in list(range(len(AZIMUTHS))) + [255, 256, 299]:
            assert _same(got[v:v + 1], _pan(ones, scalars[v], mode)), (v, scalars[v])
    assert np.all(np.isfinite(got)) and np.all(got >= -1e-6) and np.all(got <= 1.0)     # (cosf(float32(pi / 2)) = -4.4e-8)
    clipped = [v for v in range(300) if abs(scalars[v]) > 90.0]
    assert clipped and all(np.array_equal(got[v], got[1] if scalars[v] < 0 else got[6]) for v in clipped)


# ------------------------------------------------------------------------------------------ 2. pgx_pan_bank
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_pan_bank_rows_equal_pan(mode, form):
    L = lib()
    batch = len(AZIMUTHS)
    with guarded():
        for n, channels in ((1, 2), (255, 1), (257, 3), (1025, 9), (1025, 1)):
            x = _inputs(batch, n, channels, seed=7 * n + channels)
            a = _Args(x, form, mode)
            out_stride = 2 * n + PADS[1]
            filled = _pattern(batch * out_stride, 77).reshape(batch, out_stride)
            out = DeviceBuffer.from_host(filled)
            assert L.pgx_pan_bank(out.ptr, out_stride, *a.rows()) == PGX_OK, L.pgx_last_error()
            got = out.to_host()
            for v in range(batch):
                want = _pan(x[v], a.azimuth(v), mode)
                what = f"n={n} ch={channels} voice {v}"
                assert np.all(np.isfinite(want)), what
                assert _same(got[v, :2 * n].reshape(n, 2), want), what
            assert np.any(got[:, :2 * n]) and not np.array_equal(got[:, 0:2 * n:2], got[:, 1:2 * n:2])
            assert _same(got[:, 2 * n:], filled[:, 2 * n:]), f"n={n} ch={channels}: the gaps between the rows"


# ------------------------------------------------------------------------------------------ 3. pgx_pan_mix_batch
def _combinations():
    """(batch, n, channels): every value of every axis at least once, not the cross product."""
    combos = []
    for i, batch in enumerate(BATCHES):
        combos.append((batch, FRAMES[(i + 1) % len(FRAMES)], CHANNELS[i % len(CHANNELS)]))
    for i, n in enumerate(FRAMES):
        combos.append((BATCHES[(i + 3) % len(BATCHES)], n, CHANNELS[(i + 2) % len(CHANNELS)]))
    for i, channels in enumerate(CHANNELS):
        combos.append((BATCHES[(2 * i + 1) % len(BATCHES)], FRAMES[(i + 3) % len(FRAMES)], channels))
    assert {c[0] for c in combos} == set(BATCHES) and {c[1] for c in combos} == set(FRAMES)
    assert {c[2] for c in combos} == set(CHANNELS)
    return sorted(set(combos))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_pan_mix_batch_equals_pan_then_mix(mode, form):
    L = lib()
    with guarded():
        for batch, n, channels in _combinations():
            what = f"batch={batch} n={n} ch={channels}"
            x = _inputs(batch, n, channels, seed=batch * 1000 + n + channels)
            a = _Args(x, form, mode)
            # the composed path: pgx_pan per voice into [K][n][2], then pgx_mix_batch
            stacked = DeviceBuffer((batch, n, 2), np.float32)
            for v in range(batch):
                voice = DeviceBuffer.from_host(_pan(x[v], a.azimuth(v), mode))
                assert L.pgx_memcpy_d2d(stacked.offset_ptr(v * n * 2), voice.ptr, voice.nbytes) == PGX_OK
            mixed = DeviceBuffer((n, 2), np.float32)
            assert L.pgx_mix_batch(mixed.ptr, stacked.ptr, n * 2, batch, n * 2) == PGX_OK, L.pgx_last_error()
            want = mixed.to_host()
            assert np.all(np.isfinite(want)) and np.any(want), what
            assert not np.array_equal(want[:, 0], want[:, 1]), what
            out = DeviceBuffer((n, 2), np.float32)
            assert L.pgx_pan_mix_batch(out.ptr, *a.rows()) == PGX_OK, L.pgx_last_error()
            assert _same(out.to_host(), want), what


def test_a_negative_zero_survives_the_mix():
    """One voice whose samples are -0.0: the sum starts from voice 0's product, not from 0 + it."""
    L = lib()
    with guarded():
        x = np.full((1, 300, 1), -0.0, dtype=np.float32)
        a = _Args(x, "gains", 1)
        out = DeviceBuffer((300, 2), np.float32)
        assert L.pgx_pan_mix_batch(out.ptr, *a.rows()) == PGX_OK
        got = out.to_host()
    assert np.all(np.signbit(got)) and not np.any(got)
    assert _same(got, _pan(x[0], a.azimuth(0), 1))


# ------------------------------------------------------------------------------------------ 4. the argument checks
def test_nothing_to_do_and_bad_arguments():
    L = lib()
    batch, n, channels = 3, 1025, 2
    x = _inputs(batch, n, channels, seed=5)
    with guarded():
        g, s = _Args(x, "gains", 1), _Args(x, "stream", 1)
        layer_fill, mix_fill = _pattern(batch * 2 * n, 77).reshape(batch, 2 * n), _pattern(2 * n, 99).reshape(n, 2)
        layer, mixed = DeviceBuffer.from_host(layer_fill), DeviceBuffer.from_host(mix_fill)

        def call(entry, form, **changed):
            a = dict(out=(layer if entry == "pgx_pan_bank" else mixed).ptr, out_stride=2 * n, src=form.src.ptr,
                     in_stride=form.in_stride, batch=batch, n=n, channels=channels,
                     gains=form.gains.ptr if form.gains else None, az=form.az.ptr if form.az else None,
                     az_stride=form.az_stride)
            a.update(changed)
            head = (a["out"], a["out_stride"]) if entry == "pgx_pan_bank" else (a["out"],)
            return getattr(L, entry)(*head, a["src"], a["in_stride"], a["batch"], a["n"], a["channels"], a["gains"],
                                     a["az"], a["az_stride"], 1)

        for entry in ("pgx_pan_bank", "pgx_pan_mix_batch"):
            own, own_fill = (layer, layer_fill) if entry == "pgx_pan_bank" else (mixed, mix_fill)
            for form in (g, s):
                assert call(entry, form, n=0) == PGX_OK and call(entry, form, n=-4) == PGX_OK
                assert call(entry, form, batch=0) == PGX_OK and call(entry, form, batch=-1) == PGX_OK
                refused = [dict(out=None), dict(src=None), dict(channels=0), dict(channels=129),
                           dict(in_stride=n * channels - 1), dict(gains=None, az=None), dict(gains=g.gains.ptr, az=s.az.ptr)]
                if form is s:
                    refused.append(dict(az_stride=n - 1))
                if entry == "pgx_pan_bank":
                    refused += [dict(out_stride=2 * n - 1), dict(batch=65_536)]
                for changed in refused:
                    assert call(entry, form, **changed) == PGX_ERR_INVALID, (entry, changed)
                    assert entry.encode() in L.pgx_last_error(), (entry, changed)
                    assert _same(own.to_host(), own_fill), (entry, changed)         # nothing was launched
            for form in (g, s):                                   # (the same arguments, valid: it does run)
                assert call(entry, form) == PGX_OK
                got = own.to_host()
                assert np.all(np.isfinite(got)) and np.any(got)

        # pgx_pan_gains
        az = DeviceBuffer.from_host(_scalars(batch))
        gain_fill = _pattern(batch * 2, 55).reshape(batch, 2)
        gains = DeviceBuffer.from_host(gain_fill)
        assert L.pgx_pan_gains(gains.ptr, az.ptr, 0, 1) == PGX_OK and L.pgx_pan_gains(None, None, -2, 1) == PGX_OK
        for args in ((None, az.ptr), (gains.ptr, None)):
            assert L.pgx_pan_gains(*args, batch, 1) == PGX_ERR_INVALID
            assert b"pgx_pan_gains" in L.pgx_last_error()
            assert _same(gains.to_host(), gain_fill)
        assert L.pgx_pan_gains(gains.ptr, az.ptr, batch, 1) == PGX_OK
        assert np.all(np.isfinite(gains.to_host()))
