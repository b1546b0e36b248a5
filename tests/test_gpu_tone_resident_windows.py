"""
GPU: BiquadPE(SinePE) streams whose look-ahead windows are sized by the window kernel (pgx_biquad_tone_window_frames ->
BiquadPE._look_ahead_frames -> look_ahead.window_blocks).  The figure is patched to 17 000 000 frames, the smallest size
class the closed-form kernel takes; blocks are 1 000 000 frames.

* a stream of 61 blocks opens windows of 8, 16, 17 and 17 blocks (and, with its last two pulls, one more of 17: the
  first pull of a stream opens none, so 1 + 8 + 16 + 17 + 17 = 59 pulls use up four windows) and every block is the
  oracle's (np.sin + lfilter on the float32 sine) within what test_gpu_biquad_tone.py allows the same chain;
* a caller that keeps only its last snippet sees the window buffers alternate between two addresses -- what lets two live
  windows stay in the memory-side cache;
* a seek in the middle of a hinted window leaves the state and the samples where block-by-block rendering leaves them;
* pgx_biquad_tone_window (the chain's constants evaluated once, pgx_biquad_tone_plan) writes what pgx_biquad_tone
  writes, bit for bit: output, state and backup.
"""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
BLOCK = 1_000_000
HINT = 17_000_000
CHAIN = dict(freq=440.0, amp=1.0, phase=0.0, cutoff=1000.0, q=0.707)
STREAM = 61


def _pe(pg):
    pg.set_sample_rate(SR)
    pe = pg.BiquadPE(pg.SinePE(frequency=CHAIN["freq"], amplitude=CHAIN["amp"], phase=CHAIN["phase"]),
                     frequency=CHAIN["cutoff"], q=CHAIN["q"], mode=pg.BiquadMode.LOWPASS)
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    return pe, r


@pytest.fixture
def hinted(monkeypatch):
    from pygmu2_amd import biquad_pe, look_ahead
    monkeypatch.setattr(biquad_pe, "tone_window_frames", lambda: HINT)
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", True)
    monkeypatch.setattr(look_ahead, "_FRAMES_EXPLICIT", False)
    monkeypatch.setattr(look_ahead, "AHEAD_FRAMES", 1 << 25)
    monkeypatch.setattr(look_ahead, "AHEAD_FRAMES_SMALL_GRAPH", 1 << 27)
    monkeypatch.setattr(look_ahead, "AHEAD_BLOCKS", 256)
    look_ahead.set_enabled(True)
    yield look_ahead
    look_ahead.set_enabled(True)


@functools.lru_cache(maxsize=None)
def _oracle(frames):
    from oracle import pe_oracle as O
    x = O.sine_pure(0, frames, CHAIN["freq"], CHAIN["amp"], CHAIN["phase"], sr=SR)
    y = np.asarray(O.biquad_const(O.biquad_state(1), x, CHAIN["cutoff"], CHAIN["q"], "lowpass", 0.0, SR),
                   dtype=np.float64).reshape(-1)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------------------------------------ sizes and accuracy
def test_window_sizes_and_every_block_against_the_oracle(hinted):
    import pygmu2_amd as pg
    pe, r = _pe(pg)
    assert pe._look_ahead_frames() == HINT
    want = _oracle(STREAM * BLOCK)
    peak = float(np.max(np.abs(want)))
    windows, worst = [], 0.0
    for k in range(STREAM):
        before = dict(hinted.STATS)
        got = pe.render(k * BLOCK, BLOCK).data.reshape(-1)
        if hinted.STATS["windows"] != before["windows"]:
            assert hinted.STATS["windows"] == before["windows"] + 1
            windows.append((k, (hinted.STATS["window_frames"] - before["window_frames"]) // BLOCK))
        err = float(np.max(np.abs(got.astype(np.float64) - want[k * BLOCK:(k + 1) * BLOCK])))
        worst = max(worst, err)
        assert err <= 1e-6 * peak + 1e-9, (k, err, peak)
    taken = dict(pe._tone_supported)
    r.stop()
    print(f"windows (first block, blocks): {windows}; worst block {worst / peak:.3e} of peak {peak:.4f}; tone sizes {taken}")
    assert windows == [(1, 8), (9, 16), (25, 17), (42, 17), (59, 17)]
    # the 16- and 17-block windows are the closed-form kernel's; the first pull and the 8-block window are below its sizes
    assert taken == {BLOCK: False, 8 * BLOCK: False, 16 * BLOCK: True, 17 * BLOCK: True}


# ------------------------------------------------------------------------------------------------ buffers alternate
def test_window_buffers_alternate_between_two_addresses(hinted):
    """The caller keeps only its last snippet, as the benchmark does: when window k + 1 opens, window k - 1's buffer has
    just been released (its last row died with the pull that opened window k) and the LIFO pool hands it out again."""
    import pygmu2_amd as pg
    pe, r = _pe(pg)
    keep, addresses, k = None, [], 0
    while len(addresses) < 8 and k < 200:
        before = hinted.STATS["windows"]
        keep = pe.render(k * BLOCK, BLOCK)
        if hinted.STATS["windows"] != before:
            win = pe.__dict__["_la_win"]
            addresses.append(((win.end - win.first) // BLOCK, win.buf.ptr))
        k += 1
    del keep
    r.stop()
    assert [blocks for blocks, _ in addresses] == [8, 16, 17, 17, 17, 17, 17, 17]
    equal = [p for _, p in addresses[2:]]                     # six equal windows
    print("window buffers:", [hex(p) for p in equal])
    assert len(set(equal)) <= 2
    assert all(equal[i] == equal[i + 2] for i in range(4))
    assert all(p % 16 == 0 for p in equal)


# ------------------------------------------------------------------------------------------------ seek inside a window
def _seek_stream(pg, look_ahead, enabled):
    """Pulls 0 .. 29 (the 30th is the fifth block of the first 17-block window), a seek, three more blocks."""
    look_ahead.set_enabled(enabled)
    pe, r = _pe(pg)
    inside = None
    for k in range(30):
        s = pe.render(k * BLOCK, BLOCK)
    if enabled:
        win = pe.__dict__["_la_win"]
        inside = ((win.end - win.first) // BLOCK, (win.served - win.first) // BLOCK)
    del s
    far = 400 * BLOCK + 12_345
    outs = [pe.render(far + j * BLOCK, BLOCK).data.reshape(-1).copy() for j in range(4)]
    from pygmu2_amd import device
    device.synchronize()
    look_ahead.before_direct_access(pe)                       # close the window the three blocks opened: the state of a
    state = pe._state.to_host().reshape(-1).copy()            # stream that stops here
    r.stop()
    return outs, state, inside


def test_seek_in_the_middle_of_a_hinted_window(hinted):
    """The settled window puts the snapshot back and renders the five consumed blocks again, exactly; the snapshot is the
    state the window before it left, the steady solution's, which is the recurrence's to ~1e-7 of the amplitude
    (test_gpu_biquad_tone.py: 1e-6 for the state, 1e-6 of the peak for the samples that follow)."""
    import pygmu2_amd as pg
    got, state, inside = _seek_stream(pg, hinted, True)
    want, state_want, _ = _seek_stream(pg, hinted, False)
    assert inside == (17, 5)
    peak = max(float(np.max(np.abs(b))) for b in want)
    for j, (a, b) in enumerate(zip(got, want)):
        err = float(np.max(np.abs(a.astype(np.float64) - b)))
        print(f"block {j} after the seek: {err / peak:.3e} of peak {peak:.4f}")
        assert err <= 1e-6 * peak, (j, err, peak)
    print("state", state, "block by block", state_want)
    assert float(np.max(np.abs(state - state_want))) <= 1e-6, (state, state_want)


# ------------------------------------------------------------------------------------------------ the plan entry
class _Plan:
    def __init__(self, phase):
        import pygmu2_amd as pg
        from pygmu2_amd import device
        from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
        self.lib = device.ensure_init()
        self.c = rbj_coefficients(pg.BiquadMode.LOWPASS, CHAIN["cutoff"], CHAIN["q"], 0.0, float(SR))
        self.settle = settle_frames(self.c[3], self.c[4])
        self.w, self.amp, self.phase = 2.0 * np.pi * CHAIN["freq"], 0.75, phase
        self.coef = device.DeviceBuffer.from_host(np.asarray(self.c, dtype=np.float64))
        self.tables = device.DeviceBuffer((self.lib.pgx_biquad_table_doubles(),), np.float64)
        device.check(self.lib.pgx_biquad_tables(self.tables.ptr, self.coef.ptr, 1))
        self.handle = self.lib.pgx_biquad_tone_plan(float(SR), self.w, self.amp, self.phase, *self.c, self.tables.ptr,
                                                    self.settle)
        assert self.handle

    def close(self):
        assert self.lib.pgx_biquad_tone_plan_free(self.handle) == 0


@pytest.fixture(scope="module")
def plan():
    p = _Plan(0.3)
    yield p
    p.close()


def _both_entries(p, start, n, offset):
    """(output, state, backup) of pgx_biquad_tone and of pgx_biquad_tone_window on the same call, inside guard bands."""
    from guarded_alloc import guarded
    from pygmu2_amd import device
    results, pad = [], 64
    for entry in ("tone", "window"):
        with guarded():
            buf = device.DeviceBuffer((n + 2 * pad,), np.float32)          # poisoned: every float 0xFFFFFFFF
            state = device.DeviceBuffer.from_host(np.asarray([[0.25, -0.125]], dtype=np.float64))
            backup = device.DeviceBuffer((1, 2), np.float64, zero=True)
            out = buf.ptr + 4 * (pad + offset)
            if entry == "tone":
                rc = p.lib.pgx_biquad_tone(out, start, n, float(SR), p.w, p.amp, p.phase, *p.c, p.tables.ptr, p.settle,
                                           state.ptr, backup.ptr)
            else:
                rc = p.lib.pgx_biquad_tone_window(p.handle, out, start, n, state.ptr, backup.ptr)
            device.check(rc)
            host = buf.to_host().reshape(-1).view(np.uint32)
            results.append((host, state.to_host().view(np.uint64).reshape(-1), backup.to_host().view(np.uint64).reshape(-1)))
    return results


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("start", [0, 10 ** 9])
@pytest.mark.parametrize("n", [3 * 1024 + 5, 200_001])
def test_plan_entry_is_the_seventeen_argument_entry_bit_for_bit(plan, n, start, offset):
    (a, sa, ba), (b, sb, bb) = _both_entries(plan, start, n, offset)
    first = 64 + offset
    assert np.all(a[:first] == 0xFFFFFFFF) and np.all(a[first + n:] == 0xFFFFFFFF)
    assert not np.any(a[first:first + n] == 0xFFFFFFFF)
    assert np.array_equal(a, b)
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb)
    assert np.array_equal(ba.view(np.float64), [0.25, -0.125])


def test_plan_entry_declines_what_the_gate_declines(plan):
    from pygmu2_amd import device
    lib = plan.lib
    state = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((4096, 1), np.float32)
    assert lib.pgx_biquad_tone_window(plan.handle, out.ptr, 0, 2 * plan.settle - 1, state.ptr, None) == device.ERR_INVALID
    assert b"not supported" in lib.pgx_last_error()
    assert lib.pgx_biquad_tone_window(None, out.ptr, 0, 4096, state.ptr, None) == device.ERR_INVALID
    assert lib.pgx_biquad_tone_window(plan.handle, out.ptr, 4 * 10 ** 10, 4096, state.ptr, None) == device.ERR_INVALID
    assert b"fast sine range" in lib.pgx_last_error()
    assert lib.pgx_biquad_tone_window(plan.handle, out.ptr, 0, 0, state.ptr, None) == 0
    # a chain the gate declines at every length has no plan: 55 Hz into an 8 kHz high-pass
    import pygmu2_amd as pg
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    hp = rbj_coefficients(pg.BiquadMode.HIGHPASS, 8000.0, 0.707, 0.0, float(SR))
    assert not lib.pgx_biquad_tone_plan(float(SR), 2.0 * np.pi * 55.0, 1.0, 0.0, *hp, plan.tables.ptr,
                                        settle_frames(hp[3], hp[4]))
    assert np.all(state.to_host() == 0.0)
