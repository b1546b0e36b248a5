"""GPU: ReversePitchEchoPE on the device against the reference-rendered fixtures (tests/golden/reverse_echo.npz): every
case under every one of its block patterns, per block within REL_TOL * peak + ABS_FLOOR (tests/fixture_harness.py); what
the fixture has exactly silent is exactly silent; restart, reset_state(), a change of channel count, an empty render;
the example's dry/wet mix through the public names."""

import numpy as np
import pytest

import pygmu2_amd as pg
import fixture_harness as H
import reverse_echo_common as RC
from oracle.golden_cases import materialize_array
from pygmu2_amd import device

pytestmark = pytest.mark.gpu

CASES, NPZ = H.load_cases(RC.FAMILY)
BY_NAME = {c["name"]: c for c in CASES["cases"]}
EVERY = [pc for c in CASES["cases"] for pc in RC.pattern_cases(c)]
SR = 8000


@pytest.mark.parametrize("case", [pc[1] for pc in EVERY], ids=[pc[0] for pc in EVERY])
def test_device_matches_reference(case):
    H.check_case(case, NPZ, RC.build_case, tag=RC.TAG)


def render(case):
    pe, made = RC.build_case(case)
    return H.render_blocks(pe, case["sr"], case["blocks"], case.get("ops"), lambda: H.reset_all(made))


# (the dry path of the mix is never silent; the cases with gaps or ops have 500-frame blocks, and the restart test
# below looks at their silence)
WET = [c for c in CASES["cases"] if c["patterns"] and c["name"] != "dry_wet_mix"]


@pytest.mark.parametrize("case", WET, ids=[c["name"] for c in WET])
def test_silent_blocks_are_exactly_zero(case):
    """In 64-frame blocks."""
    case = dict(case, blocks=case["patterns"]["b64"])
    outs = render(case)
    stored = H.split_blocks(case, NPZ[case["name"]])
    silent = [i for i, want in stored.items() if not np.any(want)]
    assert silent, "the first echo block of a stream is silent"
    for i in silent:
        assert not np.any(outs[i]), f"{case['name']} block {i}: silent in the fixture, not on the device"


def test_restart_and_reset_behave_as_recorded():
    case = BY_NAME["reset_and_restart"]
    outs = render(case)
    stored = H.split_blocks(case, NPZ[case["name"]])
    H.assert_per_block(case["name"], outs, stored, H.REL_TOL, H.ABS_FLOOR, RC.TAG)
    assert np.any(outs[2][:160]) and np.any(stored[2][:160])             # reset_state() before block 2: nothing changes
    assert not np.any(outs[4][:160]) and np.any(outs[4][160:])           # a restart: one echo block of silence again
    # the same stretch without the reset is the same samples
    plain = render(dict(case, ops={"4": "restart"}))
    assert H.bits_equal(np.concatenate(plain), np.concatenate(outs))


class Switch(pg.ProcessingElement):
    """Whatever `active` is: a source whose channel count changes between renders."""

    def __init__(self, active):
        self.active = active

    def inputs(self):
        return [self.active]

    def channel_count(self):
        return self.active.channel_count()

    def _render(self, start, duration):
        return self.active.render(start, duration)


def started(pe, sr=SR):
    pg.set_sample_rate(sr)
    r = pg.NullRenderer(sample_rate=sr)
    r.set_source(pe)
    r.start()
    return r


def test_channel_count_change_starts_again():
    pg.set_sample_rate(SR)
    mono = materialize_array({"rng": 31, "n": 1600, "ch": 1, "scale": 0.5})
    stereo = materialize_array({"rng": 32, "n": 1600, "ch": 2, "scale": 0.5})
    switch = Switch(pg.ArrayPE(mono))
    pe = pg.ReversePitchEchoPE(switch, 0.02, 1.5, 0.8, 1.0)
    r = started(pe)
    first = np.array(pe.render(0, 800).data)
    assert first.shape == (800, 1) and np.any(first)
    switch.active = pg.ArrayPE(stereo)
    second = np.array(pe.render(800, 800).data)
    r.stop()
    fresh = pg.ReversePitchEchoPE(pg.ArrayPE(stereo), 0.02, 1.5, 0.8, 1.0)
    r = started(fresh)
    want = np.array(fresh.render(800, 800).data)
    r.stop()
    assert second.shape == (800, 2) and not np.any(second[:160]) and np.any(second[160:])
    assert H.bits_equal(second, want)


def test_empty_render_launches_nothing():
    pg.set_sample_rate(SR)
    x = materialize_array({"rng": 33, "n": 1000, "ch": 2, "scale": 0.5})
    make = lambda: pg.ReversePitchEchoPE(pg.ArrayPE(x), 0.02, 0.75, 0.6, 1.0)    # noqa: E731
    pe = make()
    r = started(pe)
    a = np.array(pe.render(0, 500).data)
    before = pe._state.to_host()
    empty = pe.render(500, 0)
    assert empty.start == 500 and empty.duration == 0 and empty.channels == 2
    # the entry point itself with n == 0: success, the carried record untouched
    L = device.ensure_init()
    rows, plen = pe._echo.shape[1], pe._pitch.shape[1]
    assert L.pgx_reverse_echo(None, None, 0, 2, float(SR), 0.02, None, 0.75, None, 0.6, None, 1.0, None, 2400,
                              pe._state.ptr, pe._echo.ptr, pe._echo.offset_ptr(rows * 2), rows, pe._pitch.ptr, plen,
                              None) == 0
    device.synchronize()
    assert pe._state.to_host().tobytes() == before.tobytes()
    assert int(before["write_idx"][0]) == 500 % 160 and int(before["prev_len"][0]) == 160
    b = np.array(pe.render(500, 500).data)
    r.stop()
    whole = make()
    r = started(whole)
    want = np.array(whole.render(0, 1000).data)
    r.stop()
    assert H.bits_equal(np.concatenate([a, b]), want)


def test_dry_wet_mix_through_the_public_names():
    """MixPE(GainPE(src, 0.5), GainPE(ReversePitchEchoPE(src, ...), 0.5)): the example's part 3."""
    case = BY_NAME["dry_wet_mix"]
    pg.set_sample_rate(case["sr"])
    src = pg.ArrayPE(materialize_array({"rng": 22, "n": 3000, "ch": 2, "scale": 0.5}))
    wet = pg.ReversePitchEchoPE(src, block_seconds=0.02, pitch_ratio=0.75, feedback=0.6, alternate_direction=1.0)
    mix = pg.MixPE(pg.GainPE(src, 0.5), pg.GainPE(wet, 0.5))
    blocks = case["patterns"]["edges"]
    outs = H.render_blocks(mix, case["sr"], blocks)
    stored = H.split_blocks(dict(case, blocks=blocks), NPZ[case["name"]])
    H.assert_per_block("dry_wet_mix_public", outs, stored, H.REL_TOL, H.ABS_FLOOR, RC.TAG)
