"""
GPU: BiquadPE(SinePE) streams whose closed-form windows keep their last block in a buffer of its own
(BiquadPE._render_window -> pgx_biquad_tone_window_split), so that a stream rewrites one window buffer.  The set-up is
test_gpu_tone_resident_windows.py's: the window figure patched to 17 000 000 frames, 1 000 000-frame blocks, 61 pulls that
open windows of 8, 16, 17, 17 and 17 blocks (first pulls 1, 9, 25, 42, 59); the oracle and its bound, 1e-6 peak + 1e-9,
are that file's too.

* a caller that keeps only its last snippet: from the second 17-block window on every window's buffer is the same address;
* a caller that also keeps an early block, or the last block, of a window across the next two openings still reads its own
  samples there (nothing writes into a buffer a snippet refers to), and the later windows are right;
* half a block inside the tail is served from it; the pull after it, which reaches beyond the window, settles the window
  and renders normally;
* a seek in the middle of a split window leaves samples and state where block-by-block rendering leaves them;
* with the switch off (biquad_pe.tone_split_tail) the window buffers alternate between two addresses, as before.
"""

import numpy as np
import pytest

import test_gpu_tone_resident_windows as base
from test_gpu_tone_resident_windows import hinted      # noqa: F401 -- the fixture

pytestmark = pytest.mark.gpu

BLOCK, STREAM = base.BLOCK, base.STREAM
OPENINGS = [(1, 8), (9, 16), (25, 17), (42, 17), (59, 17)]          # (first pull, blocks) of the stream's windows


def _want():
    want = base._oracle(STREAM * BLOCK)
    return want, float(np.max(np.abs(want)))


def _check(snippet, k, want, peak, start=None, frames=BLOCK):
    start = k * BLOCK if start is None else start
    got = snippet.data.reshape(-1)
    assert got.shape == (frames,) and snippet.start == start
    err = float(np.max(np.abs(got.astype(np.float64) - want[start:start + frames])))
    assert err <= 1e-6 * peak + 1e-9, (k, start, err, peak)


def _stream(pe, la, want, peak, keep_pulls=()):
    """61 pulls; the caller holds its last snippet and those of `keep_pulls`.  -> ([(pull, blocks, buf.ptr, tail.ptr)] of
    the windows opened, {pull: snippet kept})."""
    opened, kept, last = [], {}, None
    for k in range(STREAM):
        before = la.STATS["windows"]
        last = pe.render(k * BLOCK, BLOCK)
        if la.STATS["windows"] != before:              # (no reference to the window is kept: its buffers must be free to go)
            opened.append((k, (pe.__dict__["_la_win"].end - pe.__dict__["_la_win"].first) // BLOCK,
                           pe.__dict__["_la_win"].buf.ptr,
                           pe.__dict__["_la_win"].tail.ptr if pe.__dict__["_la_win"].tail is not None else None))
        _check(last, k, want, peak)
        if k in keep_pulls:
            kept[k] = last
    del last
    return opened, kept


def test_one_window_buffer_is_rewritten(hinted):
    import pygmu2_amd as pg
    pe, r = base._pe(pg)
    want, peak = _want()
    opened, _ = _stream(pe, hinted, want, peak)
    r.stop()
    print("windows:", [(k, b, hex(p), t and hex(t)) for k, b, p, t in opened])
    assert [(k, b) for k, b, _, _ in opened] == OPENINGS
    assert [t is not None for _, _, _, t in opened] == [False, True, True, True, True]   # 8 blocks: not the closed form
    assert opened[3][2] == opened[4][2] and opened[3][2] % 16 == 0
    # the caller still held the previous window's last block, a row of its tail, when the next window was opened
    assert opened[2][3] != opened[3][3] and opened[3][3] != opened[4][3]


@pytest.mark.parametrize("pull", [27, 41], ids=["an_early_block", "the_last_block"])
def test_a_kept_block_survives_two_further_openings(hinted, pull):
    """Pull 27 is the third block of the first 17-block window, a row of its big buffer: the next window gets another
    buffer.  Pull 41 is that window's last block, the tail: the big buffer is free and the next window takes it."""
    import pygmu2_amd as pg
    from pygmu2_amd import device
    pe, r = base._pe(pg)
    want, peak = _want()
    opened, kept = _stream(pe, hinted, want, peak, keep_pulls=(pull,))      # every later block is checked in there
    device.synchronize()
    assert [(k, b) for k, b, _, _ in opened] == OPENINGS
    snippet = kept[pull]
    assert snippet._host is not None                   # it was read once, in the stream; now the device's copy is read again
    snippet._host = None
    _check(snippet, pull, want, peak)
    r.stop()
    bufs = [p for _, _, p, _ in opened]
    if pull == 27:
        assert bufs[3] != bufs[2]                      # window 25's buffer is the kept snippet's
    else:
        assert bufs[3] == bufs[2] == bufs[4]


def test_half_a_block_inside_the_tail_and_the_pull_beyond_the_window(hinted):
    import pygmu2_amd as pg
    pe, r = base._pe(pg)
    want, peak = _want()
    for k in range(41):                                # pulls 25 .. 40 use up the big buffer of the window [25, 42)
        s = pe.render(k * BLOCK, BLOCK)
    win = pe.__dict__["_la_win"]
    assert (win.first, win.split, win.end, win.served) == (25 * BLOCK, 41 * BLOCK, 42 * BLOCK, 41 * BLOCK)
    windows = hinted.STATS["windows"]
    half = pe.render(41 * BLOCK, BLOCK // 2)
    assert half._base[0] is win.tail and half._base[1] == 0 and hinted.STATS["windows"] == windows
    assert pe.__dict__["_la_win"] is win and win.served == 41 * BLOCK + BLOCK // 2
    _check(half, 41, want, peak, frames=BLOCK // 2)
    del win, s
    beyond = pe.render(41 * BLOCK + BLOCK // 2, BLOCK)              # settles the window: 16.5 blocks are rendered again
    assert hinted.STATS["windows"] == windows + 1
    assert pe.__dict__["_la_win"].first == 41 * BLOCK + BLOCK // 2
    _check(beyond, None, want, peak, start=41 * BLOCK + BLOCK // 2)
    _check(pe.render(42 * BLOCK + BLOCK // 2, BLOCK), None, want, peak, start=42 * BLOCK + BLOCK // 2)
    r.stop()


def _seek_stream(pg, look_ahead, enabled):
    """test_gpu_tone_resident_windows._seek_stream, which also says whether the window the seek interrupts had a tail."""
    look_ahead.set_enabled(enabled)
    pe, r = base._pe(pg)
    for k in range(30):
        s = pe.render(k * BLOCK, BLOCK)
    inside = None
    if enabled:
        win = pe.__dict__["_la_win"]
        inside = ((win.end - win.first) // BLOCK, (win.served - win.first) // BLOCK, (win.split - win.first) // BLOCK,
                  win.tail is not None and win.tail.shape == (BLOCK, 1))
        del win
    del s
    far = 400 * BLOCK + 12_345
    outs = [pe.render(far + j * BLOCK, BLOCK).data.reshape(-1).copy() for j in range(4)]
    from pygmu2_amd import device
    device.synchronize()
    look_ahead.before_direct_access(pe)
    state = pe._state.to_host().reshape(-1).copy()
    r.stop()
    return outs, state, inside


def test_seek_in_the_middle_of_a_split_window(hinted):
    import pygmu2_amd as pg
    got, state, inside = _seek_stream(pg, hinted, True)
    want, state_want, _ = _seek_stream(pg, hinted, False)
    assert inside == (17, 5, 16, True)
    peak = max(float(np.max(np.abs(b))) for b in want)
    for j, (a, b) in enumerate(zip(got, want)):
        err = float(np.max(np.abs(a.astype(np.float64) - b)))
        assert err <= 1e-6 * peak, (j, err, peak)
    assert float(np.max(np.abs(state - state_want))) <= 1e-6, (state, state_want)


def test_switch_off_the_buffers_alternate(hinted, monkeypatch):
    import pygmu2_amd as pg
    from pygmu2_amd import biquad_pe
    monkeypatch.setattr(biquad_pe, "tone_split_tail", lambda: False)
    pe, r = base._pe(pg)
    keep, addresses, k = None, [], 0
    while len(addresses) < 8 and k < 200:
        before = hinted.STATS["windows"]
        keep = pe.render(k * BLOCK, BLOCK)
        if hinted.STATS["windows"] != before:
            assert pe.__dict__["_la_win"].tail is None
            addresses.append(((pe.__dict__["_la_win"].end - pe.__dict__["_la_win"].first) // BLOCK,
                              pe.__dict__["_la_win"].buf.ptr))
        k += 1
    del keep
    r.stop()
    assert [blocks for blocks, _ in addresses] == [8, 16, 17, 17, 17, 17, 17, 17]
    equal = [p for _, p in addresses[2:]]
    assert len(set(equal)) == 2
    assert all(equal[i] == equal[i + 2] and equal[i] != equal[i + 1] for i in range(4))
