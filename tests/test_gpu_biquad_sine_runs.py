"""
GPU: BiquadPE(SinePE) over window-sized blocks rendered by wave runs (csrc/pgx_biquad.hip k_biquad_sine_runs) against
the single-launch filter kernel (k_biquad_settled<.., SINE>, wave runs off) and against the oracle (np.sin +
scipy.signal.lfilter) on sections: the head, run boundaries, the tail and the last frame.  The carried state and the
look-ahead snapshot (state_backup) are the current kernel's, and a window continues seamlessly into 1 M-frame blocks.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
PARAMS = [dict(), dict(freq=3000.3, amp=0.3, phase=1.1, cutoff=2500.0, q=2.0, mode="bandpass"),
          dict(freq=5500.0, cutoff=3000.0, mode="highpass"),
          dict(freq=700.0, cutoff=1000.0, q=1.0, mode="peaking")]


def _full(kw):
    return dict(dict(freq=440.0, amp=1.0, phase=0.0, cutoff=1000.0, q=0.707, mode="lowpass"), **kw)


def _render(min_chunks, blocks, **kw):
    """Renders the blocks with the wave runs' threshold set to min_chunks (0: off, 1: every block they can take)."""
    import pygmu2_amd as pg
    from pygmu2_amd import device, look_ahead
    lib = device.ensure_init()
    p = _full(kw)
    pg.set_sample_rate(SR)
    was = lib.pgx_biquad_sine_set_runs(min_chunks)
    look_ahead.set_enabled(False)
    try:
        pe = pg.BiquadPE(pg.SinePE(frequency=p["freq"], amplitude=p["amp"], phase=p["phase"]), frequency=p["cutoff"],
                         q=p["q"], mode=pg.BiquadMode(p["mode"]))
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(pe)
        r.start()
        outs = [pe.render(s, n).data.reshape(-1).copy() for s, n in blocks]
        r.stop()
        return outs
    finally:
        look_ahead.set_enabled(True)
        lib.pgx_biquad_sine_set_runs(was)


def _close(a, b, peak):
    """Within a few float32 roundings.  How many samples differ at all is not asserted: the two kernels evaluate their
    sine anchors exactly at different frames (workgroup starts, wave starts) and turn them from there, and an exact
    anchor carries ulp(phase) of rounding, as every sample of the reference does -- 2e-3 of the samples of a 33 M-frame
    block from frame 0, more the further the stream has run."""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert float(d.max()) <= 5e-7 * peak, (float(d.max()), peak, np.count_nonzero(d) / d.size)


@pytest.mark.parametrize("n", [33_000_000, 134_000_000])
@pytest.mark.parametrize("kw", PARAMS)
def test_wave_runs_equal_the_current_kernel(kw, n):
    blocks = [(0, n)] if n < 10 ** 8 else [(10 ** 9, n)]
    new, cur = _render(1, blocks, **kw), _render(0, blocks, **kw)
    for a, b in zip(new, cur):
        _close(a, b, float(np.max(np.abs(b))))


def _oracle_section(p, s, length, settle):
    """Frames [s, s + length) of the stream: the filter forgets, so it runs from zero state 4 settle before s."""
    from oracle import pe_oracle as O
    s0 = max(0, s - 4 * settle)
    x = O.sine_pure(s0, s + length - s0, p["freq"], p["amp"], p["phase"], sr=SR)
    y = O.biquad_const(O.biquad_state(1), x, p["cutoff"], p["q"], p["mode"], 0.0, SR)
    return np.asarray(y).reshape(-1)[s - s0:]


@pytest.mark.parametrize("kw", [PARAMS[0], PARAMS[1]])
def test_wave_runs_against_the_oracle_on_sections(kw):
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    import pygmu2_amd as pg
    p = _full(kw)
    c = rbj_coefficients(pg.BiquadMode(p["mode"]), p["cutoff"], p["q"], 0.0, float(SR))
    settle = settle_frames(c[3], c[4])
    n = 134_000_000 + 777                        # a partial last chunk
    (got,) = _render(1, [(0, n)], **kw)
    # the head (from the zero state the block starts in) and the first two hundred chunks: wave 0's head, the
    # warm-ups and run boundaries of the waves after it
    head = 200 * 1024
    sections = [(0, head)]
    # run boundaries somewhere in the middle, a spread of chunk boundaries, the tail and the last frame
    sections += [(k * 1024 - 3000, 6000) for k in range(40_000, 40_200, 7)]
    sections += [(int(f) // 1024 * 1024 - 1500, 3000) for f in np.linspace(10 ** 6, n - 10 ** 6, 61)]
    sections += [(n - 300 * 1024, 300 * 1024), (n - 1, 1)]
    peak = 0.0
    checks = []
    for s, length in sections:
        want = _oracle_section(p, s, length, settle) if s else _oracle_section(p, 0, length, 0)
        peak = max(peak, float(np.max(np.abs(want))))
        checks.append((s, got[s:s + length], want))
    for s, g, w in checks:
        err = float(np.max(np.abs(g.astype(np.float64) - w)))
        assert err <= 1e-6 * peak + 1e-9, (s, err, peak)


def _direct(lib, min_chunks, start, n, state0):
    """pgx_biquad_sine called as a look-ahead window calls it: carried state in, snapshot out."""
    from pygmu2_amd import device
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    import pygmu2_amd as pg
    c = rbj_coefficients(pg.BiquadMode.LOWPASS, 1000.0, 0.707, 0.0, float(SR))
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
    backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((n, 1), np.float32)
    was = lib.pgx_biquad_sine_set_runs(min_chunks)
    try:
        device.check(lib.pgx_biquad_sine(out.ptr, start, n, float(SR), 2.0 * np.pi * 440.0, 1.0, 0.0, coef.ptr,
                                         tables.ptr, settle_frames(c[3], c[4]), state.ptr, backup.ptr))
    finally:
        lib.pgx_biquad_sine_set_runs(was)
    return out.to_host()[:, 0], state.to_host().reshape(-1), backup.to_host().reshape(-1)


def test_carried_state_and_snapshot_match_the_current_kernel():
    from pygmu2_amd import device
    lib = device.ensure_init()
    n, state0 = 134_000_000 + 5, [0.25, -0.125]
    y_new, st_new, bk_new = _direct(lib, 1, 10 ** 9, n, state0)
    y_cur, st_cur, bk_cur = _direct(lib, 0, 10 ** 9, n, state0)
    assert np.array_equal(bk_new, np.asarray(state0)) and np.array_equal(bk_cur, np.asarray(state0))
    # re-run in scipy's order from the scanned carry-in; a last frame's float32 sine may round the other way
    assert float(np.max(np.abs(st_new - st_cur))) <= 1e-6, (st_new, st_cur)
    _close(y_new, y_cur, float(np.max(np.abs(y_cur))))
    # the carried state enters the head: its first frames are the current kernel's too
    assert float(np.max(np.abs(y_new[:4096] - y_cur[:4096]))) <= 5e-7 * float(np.max(np.abs(y_cur)))


def test_window_continues_into_blocks_of_the_current_kernel():
    """A window by wave runs, then 1 M-frame blocks (the current kernel), one after a seek: the same as when the
    window too is rendered by the current kernel."""
    n = 134_000_000
    blocks = [(0, n), (n, 1_000_000), (n + 1_000_000, 1_000_000), (10 ** 9, 1_000_000)]
    new, cur = _render(1, blocks), _render(0, blocks)
    peak = max(float(np.max(np.abs(b))) for b in cur)
    for a, b in zip(new, cur):
        _close(a, b, peak)
    # and the blocks after the window against the oracle
    p = _full({})
    y = _oracle_section(p, n - 10_000, 10_000 + 2_000_000, 4096)
    assert float(np.max(np.abs(new[1][:] - y[10_000:10_000 + 1_000_000]))) <= 1e-6 * peak + 1e-9
    assert float(np.max(np.abs(new[2][:] - y[10_000 + 1_000_000:]))) <= 1e-6 * peak + 1e-9
