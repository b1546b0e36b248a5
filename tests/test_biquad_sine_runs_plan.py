"""pgx_biquad_sine_runs_plan against a Python restatement of the wave-run plan (csrc/pgx_biquad.hip
biquad_sine_runs_plan).  The plan is sized by the device's resident waves, so without a device there is no plan to
hold it against: the test skips."""

import ctypes as C

import pytest

from pygmu2_amd import device

CHUNK = 1024


def _restated(n, settle, resident, min_chunks):
    """(run, head, tail, warm, waves) or None."""
    if min_chunks <= 0 or resident <= 0 or settle <= 0:
        return None
    chunks, warm = -(-n // CHUNK), -(-settle // CHUNK)
    run = -(-chunks // resident)
    if run < min_chunks or run < 4 * warm:
        return None
    head = max(run // 2, warm)
    tail = max(run - head, 1)
    if chunks <= head + tail:
        return None
    return run, head, tail, warm, 1 + -(-(chunks - head - tail) // run)


def _export(lib, n, settle):
    out = (C.c_int * 5)(-1, -1, -1, -1, -1)
    ok = lib.pgx_biquad_sine_runs_plan(n, settle, out)
    assert ok in (0, 1) and (ok == 1 or list(out) == [-1] * 5)
    return tuple(out) if ok else None


@pytest.mark.skipif(not device.device_available(), reason="the plan is sized by the device's resident waves")
def test_runs_plan_export_is_the_restated_arithmetic():
    lib = device.ensure_init()
    was = lib.pgx_biquad_sine_set_runs(1)
    try:
        # the resident round: with a one-chunk warm-up the shortest block taken has a run of 4 chunks, 3 x resident + 1
        lo, hi = 1, 1 << 17
        assert _export(lib, hi * CHUNK, 1) is not None
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if _export(lib, mid * CHUNK, 1) is not None else (mid + 1, hi)
        assert (lo - 1) % 3 == 0
        resident = (lo - 1) // 3
        assert resident % 4 == 0 and resident >= 64
        sizes = [1, 1_000_000, lo * CHUNK - CHUNK, lo * CHUNK - CHUNK + 1, lo * CHUNK + 777, 16_000_000, 33_000_000,
                 1 << 26, 134_000_000, 134_000_000 + 777]
        for min_chunks in (1, 4, 9):
            lib.pgx_biquad_sine_set_runs(min_chunks)
            for settle in (1, 512, 1024, 1025, 5000):
                for n in sizes:
                    assert _export(lib, n, settle) == _restated(n, settle, resident, min_chunks), (n, settle, min_chunks)
        lib.pgx_biquad_sine_set_runs(0)
        assert _export(lib, 134_000_000, 512) is None
        assert _export(lib, 0, 512) is None and _export(lib, 134_000_000, 0) is None
    finally:
        lib.pgx_biquad_sine_set_runs(was)
