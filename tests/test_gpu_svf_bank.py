"""GPU: pgx_svf_bank -- pgx_svf with the voice in the grid -- against pgx_svf itself, bit for bit in samples and final
{s0, s1}: one voice at every block length where the plan changes (one tile of 1024 frames, two tiles walked by one
workgroup, three and four segments), padded rows of five voices with carried state, and the argument checks.  Five forms:
`coef` (the host's nine constants, what SVFilterPE and the voice bank pass), `const` (params only: the constants
evaluated on the device), and a per-sample cutoff, Q, or both.  Every device buffer lies between guard bands
(tests/guarded_alloc.py); the gaps between the rows of one buffer, which the guards do not see, hold a NaN pattern that
must survive."""

import numpy as np
import pytest

from guarded_alloc import guarded
from pygmu2_amd import device
from pygmu2_amd._kernels import DeviceBuffer, lib
from pygmu2_amd.svfilter_pe import _SVF_MODE_INDEX, svf_coefficients

pytestmark = pytest.mark.gpu

SR = 48000.0
PGX_OK, PGX_ERR_INVALID = 0, -1
FORMS = ("coef", "const", "freq", "q", "both")
LENGTHS = (1, 1023, 1024, 1025, 2048, 2049, 3077)
MODE_OF = {index: mode for mode, index in _SVF_MODE_INDEX.items()}


def _pattern(count, first=0):
    """float32 NaNs, no two alike (the guard bands' words)."""
    words = (np.arange(count, dtype=np.uint32) + np.uint32(first)) & np.uint32(0xFFFFF)
    return (np.uint32(0xFFF00000) | words).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _voices(batch, n, channels, seed, mode=None):
    """Per voice: input (n, channels), cutoff (n,) in 300 .. 3000 Hz, Q (n,) in 0.8 .. 3.2, mode (v % 7 unless given),
    gain_db in {-3, 0, 3}, A = 10^(gain_db/40), state {s0, s1} per channel."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = rng.uniform(-1.0, 1.0, (batch, n, channels)).astype(np.float32)
    freq = np.stack([1650.0 + 1350.0 * np.sin(0.003 * (v + 1) * t + v) for v in range(batch)]).astype(np.float32)
    q = np.stack([2.0 + 1.2 * np.cos(0.0017 * (v + 2) * t) for v in range(batch)]).astype(np.float32)
    rec = np.zeros(batch, dtype=device.BIQUAD_VAR_PARAMS)
    gains = np.zeros(batch, dtype=np.float64)
    for v in range(batch):
        gain_db = 3.0 * (v % 3) - 3.0
        rec[v] = (1500.0 + 10.0 * v, 2.0 + 0.1 * v, gain_db, v % 7 if mode is None else mode, 0)
        gains[v] = 10.0 ** (gain_db / 40.0)
    state = rng.uniform(-0.1, 0.1, (batch, channels, 2))
    return x, freq, q, rec, gains, state


def _form(form, freq, q, rec):
    """-> (freq rows or None, q rows or None, coef [batch][9] or None)"""
    coef = None
    if form == "coef":
        coef = np.array([svf_coefficients(MODE_OF[int(r["mode"])], float(r["freq"]), float(r["q"]), float(r["gain_db"]), SR)
                         for r in rec], dtype=np.float64)
    return (freq if form in ("freq", "both") else None), (q if form in ("q", "both") else None), coef


def _single(x, freq, q, coef, rec, gain, state, use_ws):
    """pgx_svf over one voice's contiguous arrays (rec: its one record) -> (samples, final state)."""
    L = lib()
    n, channels = x.shape
    out = DeviceBuffer((n, channels), np.float32)
    src = DeviceBuffer.from_host(x)
    f = DeviceBuffer.from_host(freq) if freq is not None else None
    qq = DeviceBuffer.from_host(q) if q is not None else None
    c = DeviceBuffer.from_host(coef) if coef is not None else None
    params = device.upload_structs(rec)
    st = DeviceBuffer.from_host(state)
    need = L.pgx_scan2_workspace_bytes(n, channels) if use_ws else 0
    ws = DeviceBuffer((need,), np.uint8) if need else None
    rc = L.pgx_svf(out.ptr, src.ptr, n, channels, SR, params.ptr, f.ptr if f else None, qq.ptr if qq else None,
                   float(gain), c.ptr if c else None, st.ptr, ws.ptr if ws else None)
    assert rc == PGX_OK
    return out.to_host(), st.to_host()


def _padded(rows, stride, first):
    """[batch][stride] float32: the rows' data, then the NaN pattern up to the stride."""
    batch, width = rows.shape
    buf = _pattern(batch * stride, first).reshape(batch, stride).copy()
    buf[:, :width] = rows
    return buf


def _bank(x, freq, q, coef, rec, gains, state, use_ws, pads=(0, 0, 0, 0)):
    """pgx_svf_bank over [batch] voices, rows `pads` elements longer than their data (in, out, freq, q)
    -> (the whole padded output buffer [batch][out_stride], final states)."""
    L = lib()
    batch, n, channels = x.shape
    in_stride, out_stride, f_stride, q_stride = n * channels + pads[0], n * channels + pads[1], n + pads[2], n + pads[3]
    src = DeviceBuffer.from_host(_padded(x.reshape(batch, -1), in_stride, 11))
    out = DeviceBuffer.from_host(_pattern(batch * out_stride, 77).reshape(batch, out_stride))
    f = DeviceBuffer.from_host(_padded(freq, f_stride, 23)) if freq is not None else None
    qq = DeviceBuffer.from_host(_padded(q, q_stride, 31)) if q is not None else None
    c = DeviceBuffer.from_host(coef) if coef is not None else None
    params = device.upload_structs(rec)
    g = DeviceBuffer.from_host(gains)
    st = DeviceBuffer.from_host(state)
    need = batch * L.pgx_scan2_workspace_bytes(n, channels) if use_ws else 0
    ws = DeviceBuffer((need,), np.uint8) if need else None
    rc = L.pgx_svf_bank(out.ptr, out_stride, src.ptr, in_stride, batch, n, channels, SR, params.ptr, g.ptr,
                        f.ptr if f else None, f_stride, qq.ptr if qq else None, q_stride, c.ptr if c else None, st.ptr,
                        ws.ptr if ws else None)
    assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host(), st.to_host()


def _row(a, v):
    return None if a is None else a[v]


# ------------------------------------------------------------------------------------------ 1. one voice
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_one_voice_equals_the_single_entry(form, channels):
    with guarded():
        for n in LENGTHS:
            x, freq, q, rec, gains, state = _voices(1, n, channels, seed=n + channels, mode=(n + channels) % 7)
            f, qq, coef = _form(form, freq, q, rec)
            for use_ws in (True, False):
                want, want_state = _single(x[0], _row(f, 0), _row(qq, 0), _row(coef, 0), rec[:1], gains[0], state[0], use_ws)
                got, got_state = _bank(x, f, qq, coef, rec, gains, state, use_ws)
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
                f, qq, coef = _form(form, freq, q, rec)
                pads = (7, 5, 3, 3)
                before = state.copy()
                got, state = _bank(x, f, qq, coef, rec, gains, state, use_ws, pads)
                width = n * channels
                assert got.shape == (batch, width + 5)
                for v in range(batch):
                    want, want_state[v] = _single(x[v], _row(f, v), _row(qq, v), _row(coef, v), rec[v:v + 1], gains[v],
                                                  want_state[v], use_ws)
                    what = f"call {call} voice {v} ch={channels} {form} workspace={use_ws}"
                    assert np.all(np.isfinite(want)) and np.any(want), what
                    assert _same(got[v, :width].reshape(n, channels), want), what
                    assert _same(state[v], want_state[v]), what
                    assert np.all(np.isfinite(want_state[v])) and not _same(want_state[v], before[v]), what
                # the gaps between the rows still hold the pattern they were filled with
                untouched = _pattern(batch * (width + 5), 77).reshape(batch, width + 5)
                assert _same(got[:, width:], untouched[:, width:]), f"call {call} workspace={use_ws}"


# ------------------------------------------------------------------------------------------ 3. the argument checks
def test_nothing_to_do_and_bad_arguments():
    L = lib()
    n, channels, batch = 1025, 2, 3
    x, freq, q, rec, gains, state = _voices(batch, n, channels, seed=5)
    _, _, coef = _form("coef", freq, q, rec)
    width = n * channels
    with guarded():
        src = DeviceBuffer.from_host(x)
        filled = _pattern(batch * width, 77).reshape(batch, width)
        out = DeviceBuffer.from_host(filled)
        f, qq, c = DeviceBuffer.from_host(freq), DeviceBuffer.from_host(q), DeviceBuffer.from_host(coef)
        params, g, st = device.upload_structs(rec), DeviceBuffer.from_host(gains), DeviceBuffer.from_host(state)
        here = dict(batch=batch, n=n, out_stride=width, in_stride=width, f_ptr=f.ptr, f_stride=n, q_ptr=qq.ptr, q_stride=n,
                    coef_ptr=None, gains_ptr=g.ptr, out_ptr=out.ptr, in_ptr=src.ptr, params_ptr=params.ptr, state_ptr=st.ptr)

        def call(**changed):
            a = dict(here, **changed)
            return L.pgx_svf_bank(a["out_ptr"], a["out_stride"], a["in_ptr"], a["in_stride"], a["batch"], a["n"], channels,
                                  SR, a["params_ptr"], a["gains_ptr"], a["f_ptr"], a["f_stride"], a["q_ptr"], a["q_stride"],
                                  a["coef_ptr"], a["state_ptr"], None)

        assert call(n=0) == PGX_OK
        assert call(batch=0) == PGX_OK
        assert call(n=-4) == PGX_OK and call(batch=-1) == PGX_OK
        refused = [dict(batch=65_536), dict(out_stride=width - 1), dict(in_stride=width - 1), dict(f_stride=n - 1),
                   dict(q_stride=n - 1), dict(out_ptr=None), dict(in_ptr=None), dict(params_ptr=None), dict(gains_ptr=None),
                   dict(state_ptr=None), dict(coef_ptr=c.ptr), dict(coef_ptr=c.ptr, q_ptr=None), dict(coef_ptr=c.ptr, f_ptr=None)]
        for changed in refused:
            assert call(**changed) == PGX_ERR_INVALID, changed
            assert b"pgx_svf_bank" in L.pgx_last_error()
            assert _same(out.to_host(), filled), changed       # nothing was launched
            assert _same(st.to_host(), state), changed
        assert call() == PGX_OK                                # (the same arguments, valid: it does run)
        assert np.all(np.isfinite(out.to_host()))
        assert not _same(st.to_host(), state)
        assert call(coef_ptr=c.ptr, f_ptr=None, q_ptr=None) == PGX_OK
