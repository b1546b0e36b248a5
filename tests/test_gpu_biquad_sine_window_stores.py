"""
GPU: the stores and the launch boundary of the BiquadPE(SinePE) window kernel (csrc/pgx_biquad.hip k_biquad_sine_runs).
Its full, aligned chunks leave through the kernel's own store helper; a render into a buffer offset by 4 bytes sends the
same arithmetic through the unaligned path (store_frames), so the two must agree to the bit -- a wrong offset, a dropped
row or a clobbered register of the store path shows there.  Against the single-launch filter kernel (wave runs off) and
the oracle (np.sin + scipy.signal.lfilter) the tolerances are those of test_gpu_biquad_sine_runs.py.

The block is the smallest the wave runs take on the device under test (a run of 4 x warm chunks, found through
pgx_biquad_sine_runs_plan) plus 777 frames, so the last chunk is partial: about 12.6 M frames.  Every render asserts
through the plan that the wave-run kernel, not the fallback, rendered it.
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


def _full(kw):
    return dict(dict(freq=440.0, amp=1.0, phase=0.0, cutoff=1000.0, q=0.707, mode="lowpass"), **kw)


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


def _render(lib, p, start, n, state0, *, runs=True, offset=0):
    """pgx_biquad_sine as a look-ahead window calls it.  offset: floats the output is shifted by inside its buffer
    (1: not 16-byte aligned).  Returns (frames, final state, snapshot)."""
    from pygmu2_amd import device
    c, settle = _filter(p)
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer.from_host(np.asarray(state0, dtype=np.float64).reshape(1, 2))
    backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((n + 4,), np.float32, zero=True)
    assert out.ptr % 16 == 0
    was = lib.pgx_biquad_sine_set_runs(1 if runs else 0)
    try:
        plan = (C.c_int * 5)()
        assert lib.pgx_biquad_sine_runs_plan(n, settle, plan) == (1 if runs else 0)    # which kernel renders it
        device.check(lib.pgx_biquad_sine(out.ptr + 4 * offset, start, n, float(SR), 2.0 * np.pi * p["freq"], p["amp"],
                                         p["phase"], coef.ptr, tables.ptr, settle, state.ptr, backup.ptr))
    finally:
        lib.pgx_biquad_sine_set_runs(was)
    host = out.to_host()
    assert not host[offset + n:].any()                   # nothing written past the block
    return host[offset:offset + n], state.to_host().reshape(-1), backup.to_host().reshape(-1)


def _boundaries(n, plan):
    """Chunk indices where one wave's frames end and another's begin: the first three and the last three."""
    run, head, tail, warm, waves = plan
    chunks = -(-n // CHUNK)
    starts = [head + g * run for g in range(waves - 1)] + [chunks - tail]
    assert starts == sorted(set(starts)) and starts[-1] - starts[-2] <= run, (starts[-3:], plan)
    return starts[:3] + starts[-3:]


def _exact_sections(n, plan):
    run, head, tail, warm, waves = plan
    chunks = -(-n // CHUNK)
    sections = [("wave 0's head", 0, head * CHUNK)]
    sections += [(f"run boundary at chunk {b}", (b - 1) * CHUNK, min(n, (b + 1) * CHUNK)) for b in _boundaries(n, plan)]
    sections += [("tail and partial last chunk", (chunks - tail) * CHUNK, n)]
    return sections


def _assert_same_bits(a, b, n, plan):
    for name, lo, hi in _exact_sections(n, plan):
        bad = np.flatnonzero(a[lo:hi].view(np.uint32) != b[lo:hi].view(np.uint32))
        assert bad.size == 0, (name, lo + int(bad[0]), bad.size)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))      # and everything between them


def _close(a, b, peak):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert float(d.max()) <= 5e-7 * peak, (float(d.max()), peak, int(d.argmax()))


def _lib():
    from pygmu2_amd import device
    return device.ensure_init()


@pytest.mark.parametrize("kw", PARAMS)
def test_window_stores_equal_the_unaligned_path_and_the_current_kernel(kw):
    lib, p = _lib(), _full(kw)
    n, plan = _block(lib, _filter(p)[1])
    new, _, _ = _render(lib, p, 0, n, [0.0, 0.0])
    cur, _, _ = _render(lib, p, 0, n, [0.0, 0.0], runs=False)
    _close(new, cur, float(np.max(np.abs(cur))))
    shifted, _, _ = _render(lib, p, 0, n, [0.0, 0.0], offset=1)
    _assert_same_bits(new, shifted, n, plan)


def test_carried_state_and_snapshot():
    lib, p = _lib(), _full({})
    n, plan = _block(lib, _filter(p)[1])
    state0 = [0.25, -0.125]
    y_new, st_new, bk_new = _render(lib, p, 10 ** 9, n, state0)
    y_cur, st_cur, bk_cur = _render(lib, p, 10 ** 9, n, state0, runs=False)
    assert np.array_equal(bk_new, np.asarray(state0)) and np.array_equal(bk_cur, np.asarray(state0))
    assert float(np.max(np.abs(st_new - st_cur))) <= 1e-6, (st_new, st_cur)
    _close(y_new, y_cur, float(np.max(np.abs(y_cur))))


def _oracle_section(p, s, length, settle):
    """Frames [s, s + length) of the stream: the filter forgets, so it runs from zero state 4 settle before s."""
    from oracle import pe_oracle as O
    s0 = max(0, s - 4 * settle)
    x = O.sine_pure(s0, s + length - s0, p["freq"], p["amp"], p["phase"], sr=SR)
    y = O.biquad_const(O.biquad_state(1), x, p["cutoff"], p["q"], p["mode"], 0.0, SR)
    return np.asarray(y).reshape(-1)[s - s0:]


@pytest.mark.parametrize("kw", [PARAMS[0], PARAMS[1]])
def test_window_against_the_oracle_on_sections(kw):
    lib, p = _lib(), _full(kw)
    settle = _filter(p)[1]
    n, plan = _block(lib, settle)
    run, head, tail, warm, waves = plan
    got, _, _ = _render(lib, p, 0, n, [0.0, 0.0])
    chunks = -(-n // CHUNK)
    sections = [(0, head * CHUNK)]
    sections += [(max(0, b * CHUNK - 3000), min(n, b * CHUNK + 3000) - max(0, b * CHUNK - 3000))
                 for b in _boundaries(n, plan)]
    sections += [((chunks - tail) * CHUNK - 3000, n - ((chunks - tail) * CHUNK - 3000)), (n - 1, 1)]
    checks, peak = [], 0.0
    for s, length in sections:
        want = _oracle_section(p, s, length, settle) if s else _oracle_section(p, 0, length, 0)
        peak = max(peak, float(np.max(np.abs(want))))
        checks.append((s, got[s:s + length], want))
    for s, g, w in checks:
        err = float(np.max(np.abs(g.astype(np.float64) - w)))
        assert err <= 1e-6 * peak + 1e-9, (s, err, peak)


def test_a_second_window_continues_the_first():
    """The boundary between two launches: the second window starts where the first ended, from the state it left."""
    lib, p = _lib(), _full({})
    n, plan = _block(lib, _filter(p)[1])
    first, state1, _ = _render(lib, p, 0, n, [0.0, 0.0])
    new, st_new, bk_new = _render(lib, p, n, n, state1)
    cur, st_cur, _ = _render(lib, p, n, n, state1, runs=False)
    shifted, st_shifted, _ = _render(lib, p, n, n, state1, offset=1)
    assert np.array_equal(bk_new, state1)
    _close(new, cur, float(np.max(np.abs(cur))))
    assert float(np.max(np.abs(st_new - st_cur))) <= 1e-6 and np.array_equal(st_new, st_shifted)
    _assert_same_bits(new, shifted, n, plan)
    # the two windows are one stream: the oracle across the seam
    settle = _filter(p)[1]
    want = _oracle_section(p, n - 3000, 6000, settle)
    seam = np.concatenate([first[-3000:], new[:3000]]).astype(np.float64)
    assert float(np.max(np.abs(seam - want))) <= 1e-6 * float(np.max(np.abs(want))) + 1e-9
