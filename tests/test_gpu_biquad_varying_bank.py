"""GPU: pgx_biquad_varying_bank -- pgx_biquad_varying with the voice in the grid -- against pgx_biquad_varying itself,
bit for bit in samples and final state: one voice at every block length where the plan changes (one tile of 1024
frames, two tiles walked by one workgroup, three and four segments), padded rows of five voices with carried state, and
the argument checks.  Every device buffer lies between guard bands (tests/guarded_alloc.py); the gaps between the
rows of one buffer, which the guards do not see, hold a NaN pattern that must survive."""

import math

import numpy as np
import pytest

from guarded_alloc import guarded
from pygmu2_amd import device
from pygmu2_amd._kernels import DeviceBuffer, lib

pytestmark = pytest.mark.gpu

SR = 48000.0
PGX_OK, PGX_ERR_INVALID = 0, -1
FORMS = ("freq", "q", "both")
LENGTHS = (1, 1023, 1024, 1025, 2048, 2049, 3077)


def _pattern(count, first=0):
    """float32 NaNs, no two alike (the guard bands' words)."""
    words = (np.arange(count, dtype=np.uint32) + np.uint32(first)) & np.uint32(0xFFFFF)
    return (np.uint32(0xFFF00000) | words).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _voices(batch, n, channels, seed):
    """Per voice: input (n, channels), cutoff (n,) in 300 .. 3000 Hz, Q (n,) in 0.8 .. 3.2, mode v % 8, gain_db, state."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = rng.uniform(-1.0, 1.0, (batch, n, channels)).astype(np.float32)
    freq = np.stack([1650.0 + 1350.0 * np.sin(0.003 * (v + 1) * t + v) for v in range(batch)]).astype(np.float32)
    q = np.stack([2.0 + 1.2 * np.cos(0.0017 * (v + 2) * t) for v in range(batch)]).astype(np.float32)
    rec = np.zeros(batch, dtype=device.BIQUAD_VAR_PARAMS)
    gains = np.zeros((batch, 2), dtype=np.float64)
    for v in range(batch):
        gain_db = 3.0 * (v % 3) - 3.0
        rec[v] = (1500.0 + 10.0 * v, 2.0 + 0.1 * v, gain_db, v % 8, 0)
        a = 10.0 ** (gain_db / 40.0)
        gains[v] = (a, math.sqrt(a))
    state = rng.uniform(-0.1, 0.1, (batch, channels, 4))
    return x, freq, q, rec, gains, state


def _single(x, freq, q, rec, gains, state, use_ws):
    """pgx_biquad_varying over one voice's contiguous arrays (rec: its one record) -> (samples, final state)."""
    L = lib()
    n, channels = x.shape
    out = DeviceBuffer((n, channels), np.float32)
    src = DeviceBuffer.from_host(x)
    f = DeviceBuffer.from_host(freq) if freq is not None else None
    qq = DeviceBuffer.from_host(q) if q is not None else None
    params = device.upload_structs(rec)
    st = DeviceBuffer.from_host(state)
    need = L.pgx_scan2_workspace_bytes(n, channels) if use_ws else 0
    ws = DeviceBuffer((need,), np.uint8) if need else None
    rc = L.pgx_biquad_varying(out.ptr, src.ptr, n, channels, SR, params.ptr, f.ptr if f else None, qq.ptr if qq else None,
                              float(gains[0]), float(gains[1]), st.ptr, ws.ptr if ws else None)
    assert rc == PGX_OK
    return out.to_host(), st.to_host()


def _padded(rows, stride, first):
    """[batch][stride] float32: the rows' data, then the NaN pattern up to the stride."""
    batch, width = rows.shape
    buf = _pattern(batch * stride, first).reshape(batch, stride).copy()
    buf[:, :width] = rows
    return buf


def _bank(x, freq, q, rec, gains, state, use_ws, pads=(0, 0, 0, 0)):
    """pgx_biquad_varying_bank over [batch] voices, rows `pads` elements longer than their data (in, out, freq, q)
    -> (the whole padded output buffer [batch][out_stride], final states)."""
    L = lib()
    batch, n, channels = x.shape
    in_stride, out_stride, f_stride, q_stride = n * channels + pads[0], n * channels + pads[1], n + pads[2], n + pads[3]
    src = DeviceBuffer.from_host(_padded(x.reshape(batch, -1), in_stride, 11))
    out = DeviceBuffer.from_host(_pattern(batch * out_stride, 77).reshape(batch, out_stride))
    f = DeviceBuffer.from_host(_padded(freq, f_stride, 23)) if freq is not None else None
    qq = DeviceBuffer.from_host(_padded(q, q_stride, 31)) if q is not None else None
    params = device.upload_structs(rec)
    g = DeviceBuffer.from_host(gains)
    st = DeviceBuffer.from_host(state)
    need = batch * L.pgx_scan2_workspace_bytes(n, channels) if use_ws else 0
    ws = DeviceBuffer((need,), np.uint8) if need else None
    rc = L.pgx_biquad_varying_bank(out.ptr, out_stride, src.ptr, in_stride, batch, n, channels, SR, params.ptr, g.ptr,
                                   f.ptr if f else None, f_stride, qq.ptr if qq else None, q_stride, st.ptr,
                                   ws.ptr if ws else None)
    assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host(), st.to_host()


def _form(form, freq, q):
    return (freq if form in ("freq", "both") else None), (q if form in ("q", "both") else None)


# ------------------------------------------------------------------------------------------ 1. one voice
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_one_voice_equals_the_single_entry(form, channels):
    with guarded():
        for n in LENGTHS:
            x, freq, q, rec, gains, state = _voices(1, n, channels, seed=n + channels)
            rec[0]["mode"] = (n + channels) % 8
            f, qq = _form(form, freq, q)
            for use_ws in (True, False):
                want, want_state = _single(x[0], None if f is None else f[0], None if qq is None else qq[0], rec[:1],
                                           gains[0], state[0], use_ws)
                got, got_state = _bank(x, f, qq, rec, gains, state, use_ws)
                what = f"n={n} ch={channels} {form} workspace={use_ws}"
                assert np.all(np.isfinite(want)) and np.any(want), what
                assert _same(got.reshape(n, channels), want), what
                assert _same(got_state[0], want_state), what
                assert np.all(np.isfinite(want_state)) and not _same(want_state, state[0]), what


# ------------------------------------------------------------------------------------------ 2. five voices, padded rows
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_padded_rows_of_five_voices_with_carried_state(form, channels):
    batch = 5
    with guarded():
        for use_ws in (True, False):
            state = want_state = None
            for call, n in enumerate((3077, 2049)):
                x, freq, q, rec, gains, fresh = _voices(batch, n, channels, seed=100 + call)
                if state is None:
                    state, want_state = fresh, fresh.copy()
                f, qq = _form(form, freq, q)
                pads = (7, 5, 3, 3)
                got, state = _bank(x, f, qq, rec, gains, state, use_ws, pads)
                width = n * channels
                assert got.shape == (batch, width + 5)
                for v in range(batch):
                    want, want_state[v] = _single(x[v], None if f is None else f[v], None if qq is None else qq[v],
                                                  rec[v:v + 1], gains[v], want_state[v], use_ws)
                    what = f"call {call} voice {v} ch={channels} {form} workspace={use_ws}"
                    assert np.all(np.isfinite(want)) and np.any(want), what
                    assert _same(got[v, :width].reshape(n, channels), want), what
                    assert _same(state[v], want_state[v]), what
                # the gaps between the rows still hold the pattern they were filled with
                untouched = _pattern(batch * (width + 5), 77).reshape(batch, width + 5)
                assert _same(got[:, width:], untouched[:, width:]), f"call {call} workspace={use_ws}"


# ------------------------------------------------------------------------------------------ 3. / 4. the argument checks
def test_nothing_to_do_and_bad_arguments():
    L = lib()
    n, channels, batch = 1025, 2, 3
    x, freq, q, rec, gains, state = _voices(batch, n, channels, seed=5)
    width = n * channels
    with guarded():
        src = DeviceBuffer.from_host(x)
        filled = _pattern(batch * width, 77).reshape(batch, width)
        out = DeviceBuffer.from_host(filled)
        f, qq = DeviceBuffer.from_host(freq), DeviceBuffer.from_host(q)
        params, g, st = device.upload_structs(rec), DeviceBuffer.from_host(gains), DeviceBuffer.from_host(state)

        def call(batch=batch, n=n, out_stride=width, in_stride=width, f_stride=n, gains_ptr=g.ptr, out_ptr=out.ptr):
            return L.pgx_biquad_varying_bank(out_ptr, out_stride, src.ptr, in_stride, batch, n, channels, SR, params.ptr,
                                             gains_ptr, f.ptr, f_stride, qq.ptr, n, st.ptr, None)

        assert call(n=0) == PGX_OK
        assert call(batch=0) == PGX_OK
        assert call(n=-4) == PGX_OK and call(batch=-1) == PGX_OK
        assert call(batch=65_536) == PGX_ERR_INVALID
        assert call(out_stride=width - 1) == PGX_ERR_INVALID
        assert call(in_stride=width - 1) == PGX_ERR_INVALID
        assert call(f_stride=n - 1) == PGX_ERR_INVALID
        assert call(gains_ptr=None) == PGX_ERR_INVALID
        assert call(out_ptr=None) == PGX_ERR_INVALID
        assert b"pgx_biquad_varying_bank" in L.pgx_last_error()
        assert _same(out.to_host(), filled)                 # nothing was launched
        assert _same(st.to_host(), state)
        assert call() == PGX_OK                             # (the same arguments, valid: it does run)
        assert np.all(np.isfinite(out.to_host()))
