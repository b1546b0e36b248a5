"""GPU: pgx_function_gen_bank -- pgx_function_gen_pure's sample function with the voice in the grid -- against
pgx_function_gen_pure itself, one voice at a time, and against the CPU restatement of the reference's arithmetic
(tests/control_oracle.function_gen_block), bit for bit as uint32 words.

Geometry of k_fg_bank (csrc/pgx_control.hip): a workgroup of 256 threads renders tiles of kFgBankTile = 1 024 frames,
kFgBankT = 4 per thread, whatever the channel count.  A mono row that is 16-byte aligned: a thread owns 4 consecutive frames
and stores one float4 (the row's last, partial group as scalars).  Any other row: a thread owns frames tid, tid + 256,
tid + 512, tid + 768 of the tile and stores `channels` scalar copies per frame.  Lengths: 1; 1 023, 1 024, 1 025 (one frame
either side of a workgroup's tile); 3 109 (three tiles and 37 frames: on the float4 path nine whole groups and one of one
frame, on the scalar path 37 threads with a frame of the fourth tile).  Rows 7 elements longer than their data put every
row but the first off the 16-byte grid (the scalar path of a mono row) and hold a NaN pattern that must survive; unpadded
mono rows of 1 023 and 1 025 frames are unaligned too, of 1 024 aligned.

Voices: 65 (batches of 1, 5 and 65 are the first voices of the same list), frequencies 0.01 ... 20 000 Hz, duties
including 0, 0.5, 1, -0.2 and 1.3 (the clip), phases including 0, 0.999 and 7.25; both waveforms; 1, 2 and 3 channels;
start 0, -777 and 172 800 000 (an hour at 48 kHz).  Every device buffer lies between guard bands (tests/guarded_alloc.py)."""

import numpy as np
import pytest

import control_oracle as C
from guarded_alloc import guarded
from pygmu2_amd import device
from pygmu2_amd._kernels import DeviceBuffer, lib

pytestmark = pytest.mark.gpu

SR = 48000.0
PGX_OK, PGX_ERR_INVALID = 0, -1
TILE = 1024                                         # kFgBankTile
LENGTHS = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 37)
STARTS = (0, -777, 172_800_000)
BATCHES = (1, 5, 65)
DUTIES = (0.5, 0.0, 1.0, -0.2, 1.3, 0.3, 0.77, 1e-13, 1.0 - 1e-13)
PHASES = (0.0, 0.999, 7.25, 0.25, -0.4)
WAVES = ("rectangle", "sawtooth")


def _voices(count=max(BATCHES)):
    freqs = 0.01 * (20_000.0 / 0.01) ** (np.arange(count) / (count - 1.0))
    assert freqs[0] == 0.01 and abs(freqs[-1] - 20_000.0) < 1e-6
    rec = np.zeros(count, dtype=device.FUNCTION_GEN_PARAMS)
    for v in range(count):
        rec[v] = (float(np.float64(freqs[v]) / SR), PHASES[v % len(PHASES)], DUTIES[v % len(DUTIES)])
    return freqs, rec


def _pattern(count, first=0):
    """float32 NaNs, no two alike (the guard bands' words)."""
    words = (np.arange(count, dtype=np.uint32) + np.uint32(first)) & np.uint32(0xFFFFF)
    return (np.uint32(0xFFF00000) | words).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pure(rec, start, n, channels, saw):
    """pgx_function_gen_pure, one voice at a time -> [voices][n * channels]"""
    L = lib()
    out = DeviceBuffer((n * channels,), np.float32)
    rows = []
    for r in rec:
        out.upload(_pattern(n * channels, 5))
        rc = L.pgx_function_gen_pure(out.ptr, start, n, channels, saw, float(r["dt"]), float(r["phase"]), float(r["duty"]))
        assert rc == PGX_OK, L.pgx_last_error()
        rows.append(out.to_host())
    return np.stack(rows)


def _bank(rec, start, n, channels, saw, pad):
    """pgx_function_gen_bank over rows `pad` elements longer than their data -> the whole buffer [batch][stride]"""
    L = lib()
    batch, stride = len(rec), n * channels + pad
    out = DeviceBuffer.from_host(_pattern(batch * stride, 77).reshape(batch, stride))
    params = device.upload_structs(rec)
    rc = L.pgx_function_gen_bank(out.ptr, stride, batch, start, n, channels, saw, params.ptr)
    assert rc == PGX_OK, L.pgx_last_error()
    return out.to_host()


def _oracle(freqs, rec, start, n, channels, wave):
    rows = []
    for f, r in zip(freqs, rec):
        y, _, _ = C.function_gen_block(None, start, n, np.full(n, f, dtype=np.float64), np.full(n, float(r["duty"])),
                                       float(r["phase"]), SR, wave, channels, True)
        rows.append(y.reshape(-1))
    return np.stack(rows)


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("wave", WAVES)
def test_bank_equals_the_single_entry_and_the_reference_arithmetic(wave, channels):
    freqs, rec = _voices()
    saw = int(wave == "sawtooth")
    with guarded():
        for start in STARTS:
            for n in LENGTHS:
                want = _pure(rec, start, n, channels, saw)
                assert np.all(np.abs(want) <= 1.0)                       # (every element was written: no NaN is left)
                cpu = _oracle(freqs, rec, start, n, channels, wave)
                assert np.array_equal(_bits(want), _bits(cpu)), f"pure against the CPU: {wave} ch={channels} {start} {n}"
                for batch in BATCHES:
                    for pad in (0, 7):
                        what = f"{wave} ch={channels} start={start} n={n} batch={batch} pad={pad}"
                        got = _bank(rec[:batch], start, n, channels, saw, pad)
                        assert got.shape == (batch, n * channels + pad)
                        assert np.array_equal(_bits(got[:, :n * channels]), _bits(want[:batch])), what
                        assert np.array_equal(_bits(got[:, :n * channels]), _bits(cpu[:batch])), what
                        if pad:
                            untouched = _pattern(batch * (n * channels + pad), 77).reshape(batch, -1)[:, n * channels:]
                            assert np.array_equal(_bits(got[:, n * channels:]), _bits(untouched)), f"{what}: the gaps"


def test_the_voices_differ_and_both_waveforms_move():
    """(the comparison above is not between constants)"""
    freqs, rec = _voices()
    with guarded():
        for saw in (0, 1):
            got = _bank(rec, 0, 3 * TILE + 37, 1, saw, 0)
            # (a rectangle below ~7 Hz does not change within 3 109 frames: those rows are one of two constants)
            assert len({row.tobytes() for row in got}) >= (50 if saw else 10)
            assert np.all(np.abs(got) <= 1.0) and np.any(got > 0.0) and np.any(got < 0.0)


def test_argument_checks():
    L = lib()
    _, rec = _voices(5)
    with guarded():
        n, channels = 100, 2
        out = DeviceBuffer.from_host(_pattern(5 * (n * channels + 7), 3))
        params = device.upload_structs(rec)
        before = out.to_host()
        ok = (out.ptr, n * channels + 7, 5, 0, n, channels, 1, params.ptr)
        bad = {"null out": (None,) + ok[1:], "null params": ok[:7] + (None,),
               "no channel": ok[:5] + (0,) + ok[6:], "negative channels": ok[:5] + (-1,) + ok[6:],
               "stride below the row": (out.ptr, n * channels - 1) + ok[2:],
               "batch too large": (out.ptr, n * channels, 65536) + ok[3:]}
        for what, args in bad.items():
            assert L.pgx_function_gen_bank(*args) == PGX_ERR_INVALID, what
            assert b"pgx_function_gen_bank" in L.pgx_last_error()
        # nothing to do: PGX_OK whatever the pointers, nothing launched
        assert L.pgx_function_gen_bank(None, 0, 5, 0, 0, channels, 1, None) == PGX_OK
        assert L.pgx_function_gen_bank(None, 0, 5, 0, -3, channels, 1, None) == PGX_OK
        assert L.pgx_function_gen_bank(None, 0, 0, 0, n, channels, 1, None) == PGX_OK
        assert L.pgx_function_gen_bank(None, 0, -1, 0, n, channels, 1, None) == PGX_OK
        assert np.array_equal(_bits(out.to_host()), _bits(before))
        # one voice: the stride is not read
        assert L.pgx_function_gen_bank(out.ptr, 0, 1, 0, n, channels, 1, params.ptr) == PGX_OK
        assert L.pgx_function_gen_bank(*ok) == PGX_OK
        got = out.to_host().reshape(5, -1)
        assert np.all(np.abs(got[:, :n * channels]) <= 1.0)
        assert np.array_equal(_bits(got[:, n * channels:]), _bits(before.reshape(5, -1)[:, n * channels:]))
