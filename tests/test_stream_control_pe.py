"""
GPU: ControlPE -- a constant that another thread moves between renders.  A render drains the queue and fills its block
with the last value (float32(value), as np.full does); `value` changes only when a render has consumed something.
Under TimeWarpPE a value set between two blocks of a stream changes the very next block: no window is rendered ahead
over a ControlPE.  (Named to be collected after the test_gpu_* modules, like tests/test_portamento_gpu.py.)
"""

import threading

import numpy as np
import pytest

import fixture_harness as H

pytestmark = pytest.mark.gpu

SR = 44100


@pytest.fixture(autouse=True)
def _sample_rate():
    import pygmu2_amd as pg
    pg.set_sample_rate(SR)


def _block(pe, start, n):
    return np.array(pe.render(start, n).data)


def _assert_constant(got, value, n, channels):
    assert got.dtype == np.float32 and got.shape == (n, channels)
    H.assert_bits(f"a block of {value!r}", got, np.full((n, channels), value, dtype=np.float32))


def test_initial_value():
    import pygmu2_amd as pg
    _assert_constant(_block(pg.ControlPE(), 0, 257), 0.0, 257, 1)
    c = pg.ControlPE(initial_value=0.1)
    _assert_constant(_block(c, -1000, 1), 0.1, 1, 1)
    assert c.value == 0.1


def test_set_value_then_render():
    import pygmu2_amd as pg
    c = pg.ControlPE(1.0)
    _assert_constant(_block(c, 0, 64), 1.0, 64, 1)
    c.set_value(-2.7)
    assert c.value == 1.0                                       # nothing rendered yet
    _assert_constant(_block(c, 64, 65), -2.7, 65, 1)
    assert c.value == -2.7
    _assert_constant(_block(c, 129, 1000), -2.7, 1000, 1)       # and it stays


def test_the_last_of_several_queued_values_wins():
    import pygmu2_amd as pg
    c = pg.ControlPE(0.5)
    for v in (1.0, 2.0, 3.3):
        c.set_value(v)
    assert c.value == 0.5
    _assert_constant(_block(c, 0, 63), 3.3, 63, 1)
    assert c.value == 3.3
    _assert_constant(_block(c, 63, 63), 3.3, 63, 1)


@pytest.mark.parametrize("channels", [2, 3])
def test_channels(channels):
    import pygmu2_amd as pg
    c = pg.ControlPE(0.25, channels=channels)
    assert c.channel_count() == channels
    _assert_constant(_block(c, 0, 1001), 0.25, 1001, channels)
    c.set_value(7.0)
    _assert_constant(_block(c, 1001, 5), 7.0, 5, channels)


def test_a_producer_thread_sets_values_while_the_main_thread_renders():
    import pygmu2_amd as pg
    c = pg.ControlPE(-1.0, channels=2)
    values = [float(k) + 0.5 for k in range(1000)]
    allowed = set(np.float32([-1.0] + values).tolist())

    def produce():
        for v in values:
            c.set_value(v)

    t = threading.Thread(target=produce)
    t.start()
    seen, start = [], 0
    while t.is_alive() or not seen:
        got = _block(c, start, 256)
        start += 256
        assert np.all(got == got[0, 0]) and float(got[0, 0]) in allowed, "a block is constant and holds a value that was set"
        seen.append(float(got[0, 0]))
    t.join()
    assert seen == sorted(seen)                                 # the values only ever move forward
    _assert_constant(_block(c, start, 256), values[-1], 256, 2)
    assert c.value == values[-1]


def test_a_value_set_between_two_blocks_changes_the_very_next_block():
    """TimeWarpPE(SinePE(220), rate=ControlPE(1.0)) streamed in 256-frame blocks, the rate moved before blocks 3, 4 and
    9; against the same graph whose rate is a ConstantPE, exchanged for another one at the same blocks (the tape head
    is TimeWarpPE's own state and carries over)."""
    import pygmu2_amd as pg
    block, blocks = 256, 12
    changes = {3: 0.5, 4: 2.0, 9: -0.75}

    control = pg.ControlPE(1.0)
    live = pg.TimeWarpPE(pg.SinePE(220.0), rate=control)
    segments = pg.TimeWarpPE(pg.SinePE(220.0), rate=pg.ConstantPE(1.0))
    outs = {}
    for name, pe in (("live", live), ("segments", segments)):
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(pe)
        r.start()
        got = []
        for k in range(blocks):
            if k in changes:
                if name == "live":
                    control.set_value(changes[k])
                else:
                    pe._rate = pg.ConstantPE(changes[k])
            got.append(_block(pe, k * block, block))
        r.stop()
        outs[name] = got
    for k in range(blocks):
        H.assert_bits(f"block {k}", outs["live"][k], outs["segments"][k])
    steady = pg.TimeWarpPE(pg.SinePE(220.0), rate=pg.ConstantPE(1.0))
    want = H.render_blocks(steady, SR, [[k * block, block] for k in range(blocks)])
    for k in range(blocks):                                     # the change is heard in block 3, not later and not before
        assert H.bits_equal(outs["live"][k], want[k]) == (k < 3), k
    assert control.value == -0.75
