"""GPU: NoisePE on the device against the reference-rendered fixtures (tests/golden/noise.npz) and the numpy
restatement (tests/noise_oracle.py): every stored block of every fixed case; 1 000 000-frame renders of WHITE, PINK and
BROWN; streaming in 1024-frame and odd-sized blocks; a stream that starts 2^40 + 12345 draws in; look-ahead on against
off with a seek and a reset_state() in mid-window; restarts; seed=None.

NoisePE alone, and under PEs that do not re-associate, is held to the bit in all three modes."""

import numpy as np
import pytest

import pygmu2_amd as pg
import noise_oracle as P
from fixture_harness import load_cases
from noise_gpu_common import assert_bits, check_case
from pygmu2_amd import look_ahead

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("noise")
FIXED = [c for c in CASES["cases"] if not c.get("fuzz")]
SR = 48000
LONG = 1_000_000
MODES = {m.value: m for m in pg.NoiseMode}
LONG_SEED = {"white": 0, "pink": 7, "brown": 27}


@pytest.mark.parametrize("case", FIXED, ids=[c["name"] for c in FIXED])
def test_device_matches_reference(case):
    check_case(case, NPZ)


def started(pe):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    return r


def render_blocks(make, sizes, start=0):
    pe = make()
    r = started(pe)
    outs, at = [], start
    for n in sizes:
        outs.append(pe.render(at, n).data.copy())
        at += n
    r.stop()
    return np.concatenate(outs)


# ---------------------------------------------------------------------------------------------- long renders
@pytest.mark.parametrize("mode", P.MODES)
def test_million_frames_match_the_restatement(mode):
    pg.set_sample_rate(SR)
    seed = LONG_SEED[mode]
    want = P.NoiseStream(seed, mode).render(LONG)
    if mode == "brown":                                    # the clamp ran, on both rails
        assert np.any(want == np.float32(1.0)) and np.any(want == np.float32(-1.0))
    if mode == "white":
        # what the fixture is: uniform on [-1, 1) -- mean 0 (sd 5.8e-4 at this length), variance 1/3 (sd 3.0e-4).
        # Computed from the EXPECTED samples: this documents them and cannot hide a device error.
        x = want.astype(np.float64)
        assert abs(float(np.mean(x))) < 5 * 5.8e-4 and abs(float(np.var(x)) - 1.0 / 3.0) < 5 * 3.0e-4
        assert -1.0 <= float(x.min()) and float(x.max()) < 1.0 + 1e-7
    got = render_blocks(lambda: pg.NoisePE(seed=seed, mode=MODES[mode]), [LONG])
    assert_bits(f"long_{mode}", got, want)


@pytest.mark.parametrize("mode", P.MODES)
def test_scaled_long_render_matches_the_restatement(mode):
    """The other branch of the range: four float32 roundings after the filter."""
    pg.set_sample_rate(SR)
    n = 100_000
    want = P.NoiseStream(11, mode, 100.0, 2000.0).render(n)
    got = render_blocks(lambda: pg.NoisePE(100.0, 2000.0, seed=11, mode=MODES[mode]), [n])
    assert_bits(f"scaled_{mode}", got, want)


# ---------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("sizes", ["1024", "odd"])
def test_streaming_equals_one_big_render(mode, sizes):
    pg.set_sample_rate(SR)
    total = 150 * 1024
    blocks = [1024] * 150 if sizes == "1024" else [997, 1, 2047, 64, 4099, 31] * 21 + [total - 7239 * 21]
    assert sum(blocks) == total
    make = lambda: pg.NoisePE(-0.5, 0.75, seed=99, mode=MODES[mode])            # noqa: E731
    whole = render_blocks(make, [total], start=-5000)
    parts = render_blocks(make, blocks, start=-5000)
    assert_bits(f"stream_{sizes}_{mode}", parts, whole)
    assert float(np.max(np.abs(whole))) > 1e-3


def test_starts_are_ignored():
    """A seek does not rewind the stream: renders at scattered starts are one continuing stream."""
    pg.set_sample_rate(SR)
    pe = pg.NoisePE(seed=3)
    r = started(pe)
    got = np.concatenate([pe.render(s, 128).data.copy() for s in (0, 1000, -500, 0)])
    r.stop()
    assert_bits("starts_ignored", got[:, 0], P.numpy_draws(3, 0, 512))


@pytest.mark.parametrize("seed", [0, 2 ** 100 + 7])
def test_stream_that_starts_far_in(seed):
    """2^40 + 12345 draws in: reached by the table skip-ahead, not by rendering 2^40 frames."""
    pg.set_sample_rate(SR)
    offset, n = 2 ** 40 + 12345, 70_000
    pe = pg.NoisePE(seed=seed)
    r = started(pe)
    pe.advance(offset)
    got = np.concatenate([pe.render(0, 50_000).data.copy(), pe.render(50_000, n - 50_000).data.copy()])
    r.stop()
    assert_bits(f"far_{seed}", got[:, 0], P.numpy_draws(seed, offset, n))


def test_stream_near_the_end_of_the_64_bit_count():
    pg.set_sample_rate(SR)
    offset, n = 2 ** 63 + 2 ** 62 + 9, 5000
    pe = pg.NoisePE(0.0, 1.0, seed=12345)
    r = started(pe)
    pe.advance(offset)
    got = pe.render(0, n).data.copy()
    r.stop()
    x = P.numpy_draws(12345, offset, n)
    want = ((x + np.float32(1.0)) * np.float32(0.5)) * np.float32(1.0) + np.float32(0.0)
    assert_bits("far_2_63", got[:, 0], want)


# ---------------------------------------------------------------------------------------------- look-ahead
def graphs():
    return {
        "white": lambda: pg.NoisePE(seed=5),
        "pink": lambda: pg.NoisePE(0.0, 1.0, seed=6, mode=pg.NoiseMode.PINK),
        "brown": lambda: pg.NoisePE(seed=7, mode=pg.NoiseMode.BROWN),
        "hold_of_noise": lambda: pg.SampleHoldPE(pg.NoisePE(seed=8), pg.PeriodicTrigger(375.0), 0.1),
        "mix_of_two": lambda: pg.MixPE(pg.NoisePE(seed=9, mode=pg.NoiseMode.PINK), pg.NoisePE(-0.5, 0.5, seed=10)),
    }


GRAPHS = graphs()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_look_ahead_on_equals_off_with_seek_and_reset(name):
    """40 blocks, a seek, 10 blocks, reset_state() of every NoisePE in mid-window, 10 blocks."""
    pg.set_sample_rate(SR)

    def noise_pes(pe):
        found = [pe] if isinstance(pe, pg.NoisePE) else []
        for child in pe.inputs():
            found += noise_pes(child)
        return found

    def run(flag):
        was = look_ahead.enabled()
        look_ahead.set_enabled(flag)
        try:
            before = look_ahead.STATS["windows"]
            pe = GRAPHS[name]()
            r = started(pe)
            outs = [pe.render(i * 1024, 1024).data.copy() for i in range(40)]
            outs += [pe.render(102_400 + i * 1024, 1024).data.copy() for i in range(10)]
            for m in noise_pes(pe):
                m.reset_state()
            outs += [pe.render(112_640 + i * 1024, 1024).data.copy() for i in range(10)]
            r.stop()
            return np.concatenate(outs), look_ahead.STATS["windows"] - before
        finally:
            look_ahead.set_enabled(was)

    off, windows_off = run(False)
    on, windows_on = run(True)
    assert windows_off == 0
    assert windows_on > 0, "the stream was not served from look-ahead windows"
    assert_bits(f"look_ahead_{name}", on, off)
    if name in P.MODES:      # the reset went back to the seed: the last 10 blocks repeat the first 10
        assert_bits(f"look_ahead_reset_{name}", on[50 * 1024:], on[:10 * 1024])


@pytest.mark.parametrize("mode", P.MODES)
def test_restart_reproduces_the_first_run(mode):
    pg.set_sample_rate(SR)
    pe = pg.NoisePE(seed=13, mode=MODES[mode])
    r = started(pe)
    first = [pe.render(i * 4096, 4096).data.copy() for i in range(4)]
    r.stop()
    r.start()
    second = [pe.render(i * 4096, 4096).data.copy() for i in range(4)]
    r.stop()
    assert_bits(f"restart_{mode}", np.concatenate(second), np.concatenate(first))


@pytest.mark.parametrize("mode", P.MODES)
def test_unseeded_streams_differ_and_stay_in_range(mode):
    pg.set_sample_rate(SR)
    lo, hi = 0.25, 4.0
    pe = pg.NoisePE(lo, hi, mode=MODES[mode])
    r = started(pe)
    a = pe.render(0, 20_000).data.copy()
    r.stop()
    r.start()                                                # default_rng(None) again: fresh entropy
    b = pe.render(0, 20_000).data.copy()
    r.stop()
    c = render_blocks(lambda: pg.NoisePE(lo, hi, mode=MODES[mode]), [20_000])
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # WHITE and BROWN cannot leave [-1, 1] before the range is applied.  PINK is "roughly" in it (noise_pe.py:131): what
    # bounds it is the filter's absolute gain, 0.11 * (sum of g_k / (1 - |a_k|) + 0.115926 + 0.5362) = 7.61
    reach = 7.61 if mode == "pink" else 1.0
    for x in (a, b, c):
        assert np.all(np.isfinite(x))
        assert lo + (1.0 - reach) * 0.5 * (hi - lo) <= float(x.min()) and float(x.max()) <= lo + (1.0 + reach) * 0.5 * (hi - lo)
