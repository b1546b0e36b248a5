"""
GPU: deadline pacing of the BiquadPE(SinePE) window kernel (csrc/pgx_biquad.hip k_biquad_sine_runs, RunsPace).  A paced
wave reads the wall clock once per chunk and sets its issue priority by how far it is behind the schedule the previous
window's duration gives it.  A priority changes no sample, so every check here is bit for bit: pacing on against off,
paced windows against unpaced ones, and the read-out (pgx_biquad_sine_pacing_info) says which windows were paced -- the
second and third of a stream, never the first, never one after a change of plan.  No timing is asserted beyond
0 < duration < 1 s.

The block is the one of test_gpu_biquad_sine_window_stores.py: the smallest the wave runs take on the device under test
(a run of 4 x warm chunks) plus 777 frames, about 12.6 M frames.  Pacing is per wave and per chunk: it has nothing
larger to go wrong on.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
CHUNK = 1024
PARAMS = [dict(), dict(freq=3000.3, amp=0.3, phase=1.1, cutoff=2500.0, q=2.0, mode="bandpass"),
          dict(freq=5500.0, cutoff=3000.0, mode="highpass"),
          dict(freq=700.0, cutoff=1000.0, q=1.0, mode="peaking")]
STATE0 = [0.25, -0.125]
SECOND = 10 ** 8                                         # ticks of 10 ns


def _full(kw):
    return dict(dict(freq=440.0, amp=1.0, phase=0.0, cutoff=1000.0, q=0.707, mode="lowpass"), **kw)


def _lib():
    from pygmu2_amd import device
    return device.ensure_init()


def _filter(p):
    import pygmu2_amd as pg
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    c = rbj_coefficients(pg.BiquadMode(p["mode"]), p["cutoff"], p["q"], 0.0, float(SR))
    return c, settle_frames(c[3], c[4])


def _plan(lib, n, settle):
    """(run, head, tail, warm, waves) in chunks with the wave runs forced on, or None."""
    out = (C.c_int * 5)()
    was = lib.pgx_biquad_sine_set_runs(1)
    try:
        return tuple(out) if lib.pgx_biquad_sine_runs_plan(n, settle, out) == 1 else None
    finally:
        lib.pgx_biquad_sine_set_runs(was)


_BLOCKS = {}


def _block(lib, settle):
    """The smallest block the wave runs take, plus 777 frames (a partial last chunk), and its plan."""
    if settle not in _BLOCKS:
        lo, hi = 1, 1 << 17                              # in chunks; the plan is monotone in the block's length
        assert _plan(lib, hi * CHUNK, settle) is not None
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if _plan(lib, mid * CHUNK, settle) is not None else (mid + 1, hi)
        n = (lo - 1) * CHUNK + 1 + 777
        plan = _plan(lib, n, settle)
        assert plan is not None and plan[0] == 4 * plan[3] and n % CHUNK == 778, (n, plan)
        _BLOCKS[settle] = (n, plan)
    return _BLOCKS[settle]


def _info(lib):
    """(launch id, duration in ticks, tau in ticks) of the last wave-run launch rendered with pacing on."""
    out = np.zeros(3, dtype=np.int64)
    from pygmu2_amd import device
    device.check(lib.pgx_biquad_sine_pacing_info(out.ctypes.data))
    return tuple(int(v) for v in out)


def _render(lib, p, start, n, state0, *, pacing, runs=True, offset=0):
    """pgx_biquad_sine as a look-ahead window calls it, with pacing switched on or off for this launch.  offset: floats
    the output is shifted by inside its buffer (1: not 16-byte aligned).  Returns (frames as uint32, final state,
    snapshot)."""
    from pygmu2_amd import device
    c, settle = _filter(p)
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
    backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((n + 4,), np.float32, zero=True)
    assert out.ptr % 16 == 0
    was_runs = lib.pgx_biquad_sine_set_runs(1 if runs else 0)
    was_pacing = lib.pgx_biquad_sine_set_pacing(1 if pacing else 0)
    try:
        plan = (C.c_int * 5)()
        assert lib.pgx_biquad_sine_runs_plan(n, settle, plan) == (1 if runs else 0)    # which kernel renders it
        device.check(lib.pgx_biquad_sine(out.ptr + 4 * offset, start, n, float(SR), 2.0 * np.pi * p["freq"], p["amp"],
                                         p["phase"], coef.ptr, tables.ptr, settle, state.ptr, backup.ptr))
    finally:
        lib.pgx_biquad_sine_set_runs(was_runs)
        lib.pgx_biquad_sine_set_pacing(was_pacing)
    host = out.to_host()
    assert not host[:offset].any() and not host[offset + n:].any()      # nothing written outside the block
    return host[offset:offset + n].view(np.uint32), state.to_host().reshape(-1), backup.to_host().reshape(-1)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def _stream(lib, p, sizes, *, pacing, start=0):
    """Consecutive windows of the given sizes, the state handed on; after each one (render, pacing_info)."""
    state, got = STATE0, []
    for n in sizes:
        r = _render(lib, p, start, n, state, pacing=pacing)
        got.append((r, _info(lib)))
        state, start = r[1], start + n
    return got


@pytest.mark.parametrize("kw", PARAMS)
def test_pacing_on_equals_pacing_off(kw):
    """One window, and the same window again (which the first one paces)."""
    lib, p = _lib(), _full(kw)
    n, _ = _block(lib, _filter(p)[1])
    for start in (0, 10 ** 9):
        off = _render(lib, p, start, n, STATE0, pacing=False)
        assert np.array_equal(off[2], np.asarray(STATE0))
        _same(_render(lib, p, start, n, STATE0, pacing=True), off)
        _same(_render(lib, p, start, n, STATE0, pacing=True), off)
        assert _info(lib)[2] > 0


def test_three_windows_the_second_and_third_paced():
    lib, p = _lib(), _full({})
    n, _ = _block(lib, _filter(p)[1])
    off = _stream(lib, p, [n, n, n], pacing=False)       # (a launch with pacing off also ends the history)
    on = _stream(lib, p, [n, n, n], pacing=True)
    for (r_on, _), (r_off, _) in zip(on, off):
        _same(r_on, r_off)
    assert np.array_equal(on[1][0][2], on[0][0][1]) and np.array_equal(on[2][0][2], on[1][0][1])   # snapshot = state in
    (id1, d1, tau1), (id2, d2, tau2), (id3, d3, tau3) = (info for _, info in on)
    assert tau1 == 0                                     # no history
    assert id2 == id1 + 1 and tau2 > 0                   # the first window's id accepted
    assert id3 == id2 + 1 and tau3 > 0
    assert off[2][1] == off[0][1]                        # launches with pacing off leave the read-out alone
    for d in (d1, d2, d3):
        assert 0 < d < SECOND
    assert 0 < tau2 <= d1 and 0 < tau3 <= d2             # tau: a chunk's share of the window before


def test_a_change_of_plan_runs_unpaced():
    lib, p = _lib(), _full({})
    settle = _filter(p)[1]
    a, plan_a = _block(lib, settle)
    b = a + 3 * plan_a[0] * CHUNK
    plan_b = _plan(lib, b, settle)
    assert plan_b is not None and (plan_b[0], plan_b[3], plan_b[4]) != (plan_a[0], plan_a[3], plan_a[4])
    off = _stream(lib, p, [a, b, a], pacing=False)
    on = _stream(lib, p, [a, b, a], pacing=True)
    for (r_on, _), (r_off, _) in zip(on, off):
        _same(r_on, r_off)
    assert [info[2] for _, info in on] == [0, 0, 0]
    assert on[1][1][0] == on[0][1][0] + 1 and on[2][1][0] == on[1][1][0] + 1


def test_unaligned_output_with_pacing_on():
    lib, p = _lib(), _full({})
    n, _ = _block(lib, _filter(p)[1])
    aligned = _render(lib, p, 0, n, STATE0, pacing=True)
    shifted = _render(lib, p, 0, n, STATE0, pacing=True, offset=1)
    assert _info(lib)[2] > 0                             # the shifted render was a paced one
    _same(shifted, aligned)


def test_runs_switched_off_with_pacing_on():
    lib, p = _lib(), _full({})
    n, _ = _block(lib, _filter(p)[1])
    paced = _render(lib, p, 0, n, STATE0, pacing=True)
    before = _info(lib)
    assert before[0] > 0 and 0 < before[1] < SECOND
    single = _render(lib, p, 0, n, STATE0, pacing=True, runs=False)      # asserts that the plan says: single launch
    assert _info(lib) == before
    d = np.abs(single[0].view(np.float32).astype(np.float64) - paced[0].view(np.float32).astype(np.float64))
    assert float(d.max()) <= 5e-7 * float(np.max(np.abs(single[0].view(np.float32))))
    # and that render ended the history: the next window runs unpaced
    _same(_render(lib, p, 0, n, STATE0, pacing=True), paced)
    assert _info(lib)[0] == before[0] + 1 and _info(lib)[2] == 0


def test_the_switch_returns_the_previous_value():
    lib = _lib()
    was = lib.pgx_biquad_sine_set_pacing(0)
    try:
        assert was in (0, 1)
        assert lib.pgx_biquad_sine_set_pacing(1) == 0 and lib.pgx_biquad_sine_set_pacing(-1) == 1
        default = lib.pgx_biquad_sine_set_pacing(0)
        assert default in (0, 1) and lib.pgx_biquad_sine_set_pacing(default) == 0
    finally:
        lib.pgx_biquad_sine_set_pacing(was)
