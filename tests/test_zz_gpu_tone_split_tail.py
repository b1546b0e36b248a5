"""
GPU: pgx_biquad_tone_window_split, the closed-form BiquadPE(SinePE) window kernel with the block's last tail_frames frames
stored to a buffer of their own, called through the C ABI.  For every case out[:n - tail] | out_tail[:tail], state and backup
are what pgx_biquad_tone_window writes on the same call, bit for bit, and nothing else is written: both destinations are
poisoned (0xFF), sit 64 floats inside their allocation and between guard bands (guarded_alloc), and out, allocated n frames
long, keeps its poison from the split on.

Two chains pgx_biquad_tone_supported accepts: C2 (440 Hz into a 1 kHz low-pass) and a 5.5 kHz tone over a 3 kHz
high-pass.  A workgroup renders a piece of 4096 frames; the split lies inside piece 0 (below and above settle_frames), on
a piece boundary, in the middle of a piece on and off a multiple of 4, at 0 and at n (tail = n, tail = 0), and more than a
piece in front of the end; n runs from 2 settle_frames to a few pieces, one n no multiple of 4096 and one no multiple
of 4; start is 0 or 10^9; out and out_tail each on a 16-byte boundary and 4 bytes past one.
"""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
PIECE = 4096
PAD = 64
POISON = 0xFFFFFFFF
CHAINS = {"c2_lowpass": dict(freq=440.0, cutoff=1000.0, mode="lowpass"),
          "tone_over_highpass": dict(freq=5500.0, cutoff=3000.0, mode="highpass")}


class _Chain:
    def __init__(self, freq, cutoff, mode):
        import pygmu2_amd as pg
        from pygmu2_amd import device
        from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
        self.lib = device.ensure_init()
        self.c = rbj_coefficients(pg.BiquadMode(mode), cutoff, 0.707, 0.0, float(SR))
        self.settle = settle_frames(self.c[3], self.c[4])
        self.w = 2.0 * np.pi * freq
        assert 0 < self.settle <= 1024
        assert self.lib.pgx_biquad_tone_supported(2 * self.settle, self.settle, self.w, float(SR), *self.c)
        self.coef = device.DeviceBuffer.from_host(np.asarray(self.c, dtype=np.float64))
        self.tables = device.DeviceBuffer((self.lib.pgx_biquad_table_doubles(),), np.float64)
        device.check(self.lib.pgx_biquad_tables(self.tables.ptr, self.coef.ptr, 1))
        self.handle = self.lib.pgx_biquad_tone_plan(float(SR), self.w, 0.75, 0.3, *self.c, self.tables.ptr, self.settle)
        assert self.handle


@functools.lru_cache(maxsize=None)
def _chain(name):
    return _Chain(**CHAINS[name])


@functools.lru_cache(maxsize=None)
def _whole(name, start, n):
    """(output words, state, backup) of pgx_biquad_tone_window: the reference of every split of the same call."""
    from pygmu2_amd import device
    p = _chain(name)
    out = device.DeviceBuffer((n,), np.float32)
    state = device.DeviceBuffer.from_host(np.asarray([[0.25, -0.125]], dtype=np.float64))
    backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
    device.check(p.lib.pgx_biquad_tone_window(p.handle, out.ptr, start, n, state.ptr, backup.ptr))
    res = (out.to_host().view(np.uint32), state.to_host().view(np.uint64).reshape(-1),
           backup.to_host().view(np.uint64).reshape(-1))
    for a in res:
        a.setflags(write=False)
    assert not np.any(res[0] == POISON)
    return res


def _split(name, start, n, tail, out_offset, tail_offset):
    from guarded_alloc import guarded
    from pygmu2_amd import device
    p = _chain(name)
    with guarded():
        big = device.DeviceBuffer((n + 2 * PAD,), np.float32)                  # poisoned: every word 0xFFFFFFFF
        small = device.DeviceBuffer((tail + 2 * PAD,), np.float32)
        state = device.DeviceBuffer.from_host(np.asarray([[0.25, -0.125]], dtype=np.float64))
        backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
        device.check(p.lib.pgx_biquad_tone_window_split(p.handle, big.ptr + 4 * (PAD + out_offset),
                                                        small.ptr + 4 * (PAD + tail_offset), tail, start, n, state.ptr,
                                                        backup.ptr))
        return (big.to_host().view(np.uint32), small.to_host().view(np.uint32),
                state.to_host().view(np.uint64).reshape(-1), backup.to_host().view(np.uint64).reshape(-1))


def _cases(settle):
    """(n, split): the frames [split, n) are the tail."""
    n0, n1, n2, n3 = 2 * settle, 3 * PIECE + 1000, 2 * PIECE + 1001, 4 * PIECE
    return [
        (n0, settle - 100), (n0, settle + 200), (n0, 0), (n0, n0), (n0, n0 - 1),
        (n1, settle - 100), (n1, settle + 200),                 # inside piece 0, below and above settle
        (n1, PIECE), (n1, 2 * PIECE), (n1, 3 * PIECE),          # on a piece boundary
        (n1, PIECE + 2000), (n1, PIECE + 2001),                 # mid-piece, on and off a multiple of 4
        (n1, 3 * PIECE + 500), (n1, 3 * PIECE + 997),           # inside the block's last, short piece
        (n1, 0), (n1, n1),                                      # tail = n, tail = 0
        (n1, 100), (n1, 4),                                     # a tail of more than one piece (three of them)
        (n2, PIECE), (n2, PIECE + 2000), (n2, PIECE + 2001), (n2, 2 * PIECE + 999), (n2, 3),
        (n3, 3 * PIECE), (n3, 3 * PIECE + 2), (n3, PIECE - 4), (n3, n3 - 1),
    ]


@pytest.mark.parametrize("offsets", [(0, 0), (0, 1), (1, 0)], ids=["aligned", "tail_plus4bytes", "out_plus4bytes"])
@pytest.mark.parametrize("start", [0, 10 ** 9])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_split_is_the_whole_window_bit_for_bit(name, start, offsets):
    p = _chain(name)
    out_offset, tail_offset = offsets
    for n, split in _cases(p.settle):
        tail = n - split
        want, state_want, backup_want = _whole(name, start, n)
        big, small, state, backup = _split(name, start, n, tail, out_offset, tail_offset)
        at = (name, start, n, split, offsets)
        first = PAD + out_offset
        assert np.array_equal(big[first:first + split], want[:split]), at
        assert np.all(big[:first] == POISON) and np.all(big[first + split:] == POISON), at     # nothing past the split
        first = PAD + tail_offset
        assert np.array_equal(small[first:first + tail], want[split:]), at
        assert np.all(small[:first] == POISON) and np.all(small[first + tail:] == POISON), at
        assert np.array_equal(state, state_want) and np.array_equal(backup, backup_want), at
        assert np.array_equal(backup.view(np.float64), [0.25, -0.125]), at


def test_invalid_arguments():
    from pygmu2_amd import device
    p = _chain("c2_lowpass")
    lib, n = p.lib, 2 * PIECE
    state = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((n, 1), np.float32)
    tail = device.DeviceBuffer((n, 1), np.float32)
    out.zero_()
    tail.zero_()
    split = lib.pgx_biquad_tone_window_split
    assert split(p.handle, out.ptr, tail.ptr, -1, 0, n, state.ptr, None) == device.ERR_INVALID
    assert split(p.handle, out.ptr, tail.ptr, n + 1, 0, n, state.ptr, None) == device.ERR_INVALID
    assert split(p.handle, out.ptr, None, 1, 0, n, state.ptr, None) == device.ERR_INVALID
    assert split(p.handle, out.ptr, None, n, 0, n, state.ptr, None) == device.ERR_INVALID
    assert split(None, out.ptr, tail.ptr, PIECE, 0, n, state.ptr, None) == device.ERR_INVALID
    assert split(p.handle, out.ptr, tail.ptr, 8, 0, 2 * p.settle - 1, state.ptr, None) == device.ERR_INVALID
    assert b"not supported" in lib.pgx_last_error()
    assert split(p.handle, out.ptr, tail.ptr, 0, 0, 0, state.ptr, None) == 0
    assert split(p.handle, out.ptr, None, 0, 0, n, state.ptr, None) == 0         # tail_frames == 0: the existing entry
    device.synchronize()
    assert np.all(tail.to_host() == 0.0)
    assert lib.pgx_biquad_tone_split_tail() in (0, 1)
