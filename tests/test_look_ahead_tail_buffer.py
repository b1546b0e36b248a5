"""CPU: look-ahead windows whose root renders the window itself and hands the last block back in a buffer of its own
(`_render_window(start, duration, blocks)` -> (Snippet of the first blocks - 1 blocks, buffer of the last) or None).  A fake
window root and fake buffers (no device): the hook is asked only when offered, None gives the old path, a pull is served
from `buf`, from the tail, or -- lying across the two -- not at all (the window is settled and the pull renders
normally), STATS counts the whole window, and a window that is popped drops both buffers.  And the native switch,
pgx_biquad_tone_split_tail under PGX_TONE_SPLIT_TAIL (read once: fresh child processes, no device needed)."""

import gc
import os
import subprocess
import sys
import weakref

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import look_ahead
from pygmu2_amd.device import DeviceBuffer
from pygmu2_amd.processing_element import ProcessingElement
from pygmu2_amd.snippet import Snippet

BLOCK = 100
BORN = []                                                     # weak references to every fake buffer made


def _buffer(frames):
    """A DeviceBuffer nobody allocated: the bookkeeping only looks at its shape."""
    buf = object.__new__(DeviceBuffer)
    buf.shape, buf.dtype, buf.nbytes, buf.ptr, buf._owner = (int(frames), 1), np.dtype(np.float32), 4 * int(frames), 0, None
    BORN.append(weakref.ref(buf))
    return buf


class _Root(ProcessingElement):
    """Counts frames: its state is the frame the next render has to start at."""
    _LOOK_AHEAD_SAFE = True
    _STATE_FIELDS = ("_next",)

    def __init__(self, hook):
        self._next = 0
        self.renders, self.asked = [], []
        if hook is not None:
            self._render_window = lambda start, duration, blocks: self._own_window(hook, start, duration, blocks)

    def inputs(self):
        return []

    def _render(self, start, duration):
        self.renders.append((start, duration))
        self._next = start + duration
        return Snippet(start, _buffer(duration))

    def _own_window(self, hook, start, duration, blocks):
        self.asked.append((start, duration, blocks))
        if hook == "declines":
            return None
        self._next = start + duration * blocks
        return Snippet(start, _buffer(duration * (blocks - 1))), _buffer(duration)


@pytest.fixture
def la(monkeypatch):
    pg.set_sample_rate(44100)
    monkeypatch.setattr(look_ahead, "_FRAMES_EXPLICIT", False)
    monkeypatch.setattr(look_ahead, "AHEAD_BLOCKS", 256)
    monkeypatch.setattr(look_ahead, "FIRST_WINDOW_BLOCKS", 4)
    look_ahead.set_enabled(True)
    del BORN[:]
    yield look_ahead
    look_ahead.set_enabled(True)


def _where(snippet):
    """(buffer, first row) a served snippet is a view of."""
    return snippet._base


def _open(pe, la):
    """The first pull of a stream opens no window, the second opens one of FIRST_WINDOW_BLOCKS blocks at BLOCK."""
    pe.render(0, BLOCK)
    assert "_la_win" not in pe.__dict__
    first = pe.render(BLOCK, BLOCK)
    return pe.__dict__["_la_win"], first


def test_a_root_without_the_hook_is_not_asked_and_has_no_tail(la):
    pe = _Root(None)
    before = dict(la.STATS)
    win, first = _open(pe, la)
    assert pe.asked == [] and pe.renders == [(0, BLOCK), (BLOCK, 4 * BLOCK)]
    assert win.tail is None and (win.first, win.split, win.end) == (BLOCK, 5 * BLOCK, 5 * BLOCK)
    assert win.buf.shape == (4 * BLOCK, 1) and _where(first) == (win.buf, 0)
    assert la.STATS["window_frames"] - before["window_frames"] == 4 * BLOCK and la.STATS["windows"] - before["windows"] == 1
    for k in range(2, 5):
        assert _where(pe.render(k * BLOCK, BLOCK)) == (win.buf, (k - 1) * BLOCK)
    assert pe.renders == [(0, BLOCK), (BLOCK, 4 * BLOCK)]


def test_a_hook_that_declines_gives_the_old_path(la):
    pe = _Root("declines")
    win, first = _open(pe, la)
    assert pe.asked == [(BLOCK, BLOCK, 4)] and pe.renders == [(0, BLOCK), (BLOCK, 4 * BLOCK)]
    assert win.tail is None and win.split == win.end == 5 * BLOCK and _where(first) == (win.buf, 0)


def test_pulls_are_served_from_buf_then_from_the_tail_and_the_whole_window_is_counted(la):
    pe = _Root("splits")
    before = dict(la.STATS)
    win, first = _open(pe, la)
    assert pe.asked == [(BLOCK, BLOCK, 4)] and pe.renders == [(0, BLOCK)]
    assert (win.first, win.split, win.end, win.served) == (BLOCK, 4 * BLOCK, 5 * BLOCK, 2 * BLOCK)
    assert win.buf.shape == (3 * BLOCK, 1) and win.tail.shape == (BLOCK, 1)
    assert la.STATS["window_frames"] - before["window_frames"] == 4 * BLOCK and la.STATS["windows"] - before["windows"] == 1
    assert _where(first) == (win.buf, 0)
    assert _where(pe.render(2 * BLOCK, BLOCK)) == (win.buf, BLOCK)
    assert _where(pe.render(3 * BLOCK, BLOCK)) == (win.buf, 2 * BLOCK)
    last = pe.render(4 * BLOCK, BLOCK)
    assert _where(last) == (win.tail, 0) and (last.start, last.duration) == (4 * BLOCK, BLOCK)
    assert win.served == win.end and pe.renders == [(0, BLOCK)]
    # the pull after the window's last block continues the stream: the next window (8 blocks) opens at once
    nxt = pe.render(5 * BLOCK, BLOCK)
    assert pe.asked[-1] == (5 * BLOCK, BLOCK, 8) and _where(nxt) == (pe.__dict__["_la_win"].buf, 0)


def test_half_blocks_inside_the_tail_and_a_pull_across_the_split(la):
    pe = _Root("splits")
    win, _ = _open(pe, la)
    half = BLOCK // 2
    pe.render(2 * BLOCK, BLOCK)
    pe.render(3 * BLOCK, BLOCK)
    assert _where(pe.render(4 * BLOCK, half)) == (win.tail, 0)
    assert _where(pe.render(4 * BLOCK + half, half)) == (win.tail, half)
    assert win.served == win.end
    # a second stream of blocks that do not land on the split: the pull that lies across it settles the window (the
    # snapshot goes back and the consumed part is rendered again) and takes the normal path
    pe = _Root("splits")
    win, _ = _open(pe, la)
    odd = 3 * BLOCK // 2
    assert _where(pe.render(2 * BLOCK, odd)) == (win.buf, BLOCK)                     # [200, 350) of [100, 400) | [400, 500)
    del pe.renders[:]
    got = pe.render(2 * BLOCK + odd, odd)                                            # [350, 500): across 400
    assert "_la_win" not in pe.__dict__ or pe.__dict__["_la_win"] is not win
    assert pe.renders[0] == (BLOCK, BLOCK + odd)                                     # settle: [100, 350) again
    assert (got.start, got.duration) == (2 * BLOCK + odd, odd)
    assert pe._next >= 2 * BLOCK + 2 * odd


def test_a_seek_settles_a_split_window(la):
    pe = _Root("splits")
    win, _ = _open(pe, la)
    pe.render(2 * BLOCK, BLOCK)
    del pe.renders[:]
    pe.render(50 * BLOCK, BLOCK)
    assert pe.renders == [(BLOCK, 2 * BLOCK), (50 * BLOCK, BLOCK)] and "_la_win" not in pe.__dict__
    assert pe._next == 51 * BLOCK


def test_popping_the_window_drops_both_buffers(la):
    pe = _Root("splits")
    win, first = _open(pe, la)
    buf, tail = weakref.ref(win.buf), weakref.ref(win.tail)
    del first
    for k in range(2, 4):
        pe.render(k * BLOCK, BLOCK)
    last = pe.render(4 * BLOCK, BLOCK)
    del win
    gc.collect()
    assert buf() is not None and tail() is not None            # the window holds them
    # the caller keeps its last snippet, a row of the tail, while the next window opens: `buf` is gone before the next
    # window's buffers are made, the tail lives as long as the snippet
    made_before = len(BORN)
    seen = []
    hook = pe._render_window
    pe._render_window = lambda *a: (seen.append(buf() is None), hook(*a))[1]
    nxt = pe.render(5 * BLOCK, BLOCK)
    assert seen == [True] and len(BORN) == made_before + 2
    assert tail() is not None and _where(last)[0] is tail()
    del last
    gc.collect()
    assert tail() is None
    # ... and a caller that keeps an earlier row keeps `buf`
    win = pe.__dict__["_la_win"]
    buf, tail = weakref.ref(win.buf), weakref.ref(win.tail)
    del win
    look_ahead.settle(pe)
    gc.collect()
    assert buf() is not None and tail() is None                # `nxt` is a row of buf; nobody holds the tail
    del nxt
    gc.collect()
    assert buf() is None


@pytest.mark.parametrize("value, want", [(None, 1), ("0", 0), ("1", 1), ("", 1), ("00", 1), ("no", 1)])
def test_the_switch_is_read_in_a_fresh_process(value, want):
    """PGX_TONE_SPLIT_TAIL=0 and nothing else says "no split wanted"."""
    from pygmu2_amd.build import build
    build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "PGX_TONE_SPLIT_TAIL"}
    if value is not None:
        env["PGX_TONE_SPLIT_TAIL"] = value
    code = ("import ctypes; from pygmu2_amd.build import LIB_PATH; L = ctypes.CDLL(LIB_PATH); "
            "print(L.pgx_biquad_tone_split_tail(), L.pgx_biquad_tone_split_tail())")
    assert subprocess.check_output([sys.executable, "-c", code], env=env, cwd=root, text=True).split() == [str(want)] * 2


def test_biquad_pe_offers_the_hook_and_other_roots_do_not():
    assert hasattr(pg.BiquadPE(pg.SinePE(frequency=440.0), frequency=1000.0, q=0.707), "_render_window")
    assert not hasattr(pg.SinePE(frequency=440.0), "_render_window")
    assert not hasattr(pg.GainPE(pg.SinePE(frequency=440.0), gain=0.5), "_render_window")
