"""GPU: pgx_periodic_trigger_bank -- K PeriodicTrigger rows in one launch -- against pgx_periodic_trigger row by row, bit
for bit (and against the integer rule itself, (frame + phase_samples) % period == 0), then pgx_adsr_triggered with
batch = 5 over such rows against five batch = 1 calls, bit for bit in samples and carried state, over two consecutive
blocks.  Padded rows: the gaps hold a NaN pattern that must survive; every device buffer lies between guard bands
(tests/guarded_alloc.py)."""

import numpy as np
import pytest

from guarded_alloc import guarded
from pygmu2_amd import device
from pygmu2_amd._kernels import DeviceBuffer, lib

pytestmark = pytest.mark.gpu

PGX_OK, PGX_ERR_INVALID = 0, -1
LENGTHS = (1, 64, 1025)
LONG_PERIOD = 6857
PAD = 5


def _pattern(count, first=0):
    words = (np.arange(count, dtype=np.uint32) + np.uint32(first)) & np.uint32(0xFFFFF)
    return (np.uint32(0xFFF00000) | words).view(np.float32)


def _same(a, b):
    view = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view))


def _records(voices):
    """[(period, phase_samples, amplitude)] -> the entry's three per-voice arrays, on the host"""
    return (np.array([v[0] for v in voices], dtype=np.int64), np.array([v[1] for v in voices], dtype=np.int64),
            np.array([v[2] for v in voices], dtype=np.float32))


def _single_trigger(start, n, period, phase, amplitude):
    out = DeviceBuffer.from_host(_pattern(n, 3))
    assert lib().pgx_periodic_trigger(out.ptr, start, n, period, phase, amplitude) == PGX_OK
    return out.to_host()


def _trigger_bank(start, n, rec, pad=PAD):
    """-> (the device buffer [K][n + pad] the bank wrote into a NaN pattern, its host copy)"""
    k, stride = len(rec[0]), n + pad
    out = DeviceBuffer.from_host(_pattern(k * stride, 77).reshape(k, stride))
    periods, phases, amplitudes = (DeviceBuffer.from_host(a) for a in rec)
    rc = lib().pgx_periodic_trigger_bank(out.ptr, stride, k, start, n, periods.ptr, phases.ptr, amplitudes.ptr)
    assert rc == PGX_OK, lib().pgx_last_error()
    return out, out.to_host()


def _rule(start, n, period, phase, amplitude):
    frames = np.arange(start, start + n, dtype=np.int64) + phase
    return np.where(frames % period == 0, np.float32(amplitude), np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. the trigger rows
@pytest.mark.parametrize("n", LENGTHS)
def test_rows_equal_the_single_trigger(n):
    periods = (1, 7, n, n + 1, LONG_PERIOD)
    voices = [(period, phase, amplitude) for period in periods for phase, amplitude in ((0, 1.0), (period - 1, -2.0))]
    rec = _records(voices)
    # the long period with phase 0 fires at the multiples of LONG_PERIOD: once on frame 0, once on frame n - 1
    starts = (-5000, 0, 3 * LONG_PERIOD, 3 * LONG_PERIOD - (n - 1))
    with guarded():
        for start in starts:
            _, got = _trigger_bank(start, n, rec)
            assert got.shape == (len(voices), n + PAD)
            for v, (period, phase, amplitude) in enumerate(voices):
                want = _single_trigger(start, n, period, phase, amplitude)
                what = f"n={n} start={start} period={period} phase={phase}"
                assert _same(want, _rule(start, n, period, phase, amplitude)), what
                assert _same(got[v, :n], want), what
            assert np.all(got[0, :n] == 1.0) and np.all(got[1, :n] == -2.0)          # period 1: every frame, not silent
            untouched = _pattern(len(voices) * (n + PAD), 77).reshape(len(voices), n + PAD)
            assert _same(got[:, n:], untouched[:, n:]), f"n={n} start={start}: the gaps"
        long_row = voices.index((LONG_PERIOD, 0, 1.0))
        assert _trigger_bank(starts[2], n, rec)[1][long_row, 0] == 1.0                # an event on frame 0
        assert _trigger_bank(starts[3], n, rec)[1][long_row, n - 1] == 1.0            # ... and on frame n - 1
        if n > 1:
            assert np.count_nonzero(_trigger_bank(starts[3], n, rec)[1][long_row, :n]) == 1


def test_nothing_to_do_and_bad_arguments():
    L = lib()
    n, k = 64, 3
    rec = _records([(7, 0, 1.0), (1, 0, 1.0), (64, 63, 2.0)])
    with guarded():
        filled = _pattern(k * n, 77).reshape(k, n)
        out = DeviceBuffer.from_host(filled)
        p = [DeviceBuffer.from_host(a).ptr for a in rec]
        assert L.pgx_periodic_trigger_bank(out.ptr, n, k, 0, 0, *p) == PGX_OK
        assert L.pgx_periodic_trigger_bank(out.ptr, n, 0, 0, n, *p) == PGX_OK
        assert L.pgx_periodic_trigger_bank(out.ptr, n, 65_536, 0, n, *p) == PGX_ERR_INVALID
        assert L.pgx_periodic_trigger_bank(out.ptr, n - 1, k, 0, n, *p) == PGX_ERR_INVALID
        assert L.pgx_periodic_trigger_bank(None, n, k, 0, n, *p) == PGX_ERR_INVALID
        for missing in range(3):
            assert L.pgx_periodic_trigger_bank(out.ptr, n, k, 0, n, *[None if i == missing else p[i] for i in range(3)]) \
                == PGX_ERR_INVALID
        assert b"pgx_periodic_trigger_bank" in L.pgx_last_error()
        assert _same(out.to_host(), filled)                   # nothing was launched
        assert L.pgx_periodic_trigger_bank(out.ptr, n, k, 0, n, *p) == PGX_OK
        assert np.all(np.isfinite(out.to_host()))


# ------------------------------------------------------------------------------------------ 2. the envelopes over the rows
N = 1025
START = 3 * LONG_PERIOD - 10                 # voice 0's trigger (period 6857, phase 0) falls on frame 10 of the first block
SUSTAIN_LEVEL = 0.6


def _adsr_records():
    """Slopes per sample: attack 20 frames, decay 30.  Voice 0: sustain from frame ~60 for 1200 frames -- it ends inside the
    second block.  Voice 1 (a trigger every 700 frames: frames 0, 700, 1400): sustain 100 frames, release 1000 frames --
    still falling when the next trigger comes.  Voices 2 .. 4: a trigger every 7 frames, every frame, none in these
    blocks but one (period N + 1)."""
    rec = np.zeros(5, dtype=device.ADSR_PARAMS)
    for v, (sustain, release) in enumerate(((1200, 1500), (100, 1000), (40, 50), (10, 20), (200, 400))):
        rec[v]["attack_dvdt"] = (1.0 - 0.0) / 20.0
        rec[v]["decay_dvdt"] = (SUSTAIN_LEVEL - 1.0) / 30.0
        rec[v]["release_dvdt"] = (0.0 - SUSTAIN_LEVEL) / release
        rec[v]["sustain_level"] = SUSTAIN_LEVEL
        rec[v]["sustain_samples"] = sustain
    return rec


def _adsr(trig, trig_stride, out_stride, k, start, n, rec, state):
    """pgx_adsr_triggered over k rows -> ([k][out_stride] host copy of a NaN-patterned output, final states)"""
    L = lib()
    out = DeviceBuffer.from_host(_pattern(k * out_stride, 55).reshape(k, out_stride))
    params = device.upload_structs(rec)
    st = DeviceBuffer.from_host(state)
    ws = DeviceBuffer((L.pgx_adsr_workspace_bytes(k, n),), np.uint8)
    rc = L.pgx_adsr_triggered(out.ptr, out_stride, trig.ptr, trig_stride, k, start, n, params.ptr, st.ptr, ws.ptr)
    assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host(), st.to_host()


def test_triggered_envelopes_batched_over_the_rows_equal_one_by_one():
    triggers = _records([(LONG_PERIOD, 0, 1.0), (700, (-START) % 700, 1.0), (7, 3, 1.0), (1, 0, 1.0), (N + 1, N, 2.0)])
    rec = _adsr_records()
    with guarded():
        state = np.zeros((5, 3), dtype=np.float64)
        want_state = state.copy()
        wants = []
        for block, start in enumerate((START, START + N)):
            rows, rows_host = _trigger_bank(start, N, triggers, pad=3)
            before = state.copy()
            got, state = _adsr(rows, N + 3, N + PAD, 5, start, N, rec, state)
            want = np.zeros((5, N), dtype=np.float32)
            for v in range(5):
                row = DeviceBuffer.from_host(np.ascontiguousarray(rows_host[v, :N]))
                one, one_state = _adsr(row, N, N, 1, start, N, rec[v:v + 1], want_state[v:v + 1])
                want[v], want_state[v] = one[0], one_state[0]
                what = f"block {block} voice {v}"
                assert np.all(np.isfinite(want[v])) and np.any(want[v]), what
                assert _same(got[v, :N], want[v]), what
                assert _same(state[v], want_state[v]), what
            assert np.all(np.isfinite(state)) and not _same(state, before)
            untouched = _pattern(5 * (N + PAD), 55).reshape(5, N + PAD)
            assert _same(got[:, N:], untouched[:, N:]), f"block {block}: the gaps"
            wants.append(want)
            if block == 0:
                # voice 0 holds its sustain across the block boundary: the deadline it carries lies in the second block
                assert START + N <= want_state[0, 2] < START + 2 * N
                assert want[0, N - 1] == np.float32(SUSTAIN_LEVEL)
        # ... and has passed at the end of it: the envelope is below the sustain level, falling
        assert 0.0 < wants[1][0, N - 1] < wants[1][0, N - 2] < np.float32(SUSTAIN_LEVEL)
        # voice 1 is retriggered on frame 1400 (frame 375 of the second block) while it is being released
        env, at = wants[1][1], 1400 - N
        assert 0.0 < env[at] < env[at - 1] < env[at - 2] < np.float32(SUSTAIN_LEVEL)
        assert env[at + 2] > env[at + 1] > env[at]
