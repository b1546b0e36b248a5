"""GPU: SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE on the device against the reference-rendered
fixtures (tests/golden/control.npz) and the numpy restatement (tests/control_oracle.py): every stored block; long
renders (several workgroup segments, all-windows slew solve and its sequential fallback); streaming in 1024-frame
and odd-sized blocks; look-ahead on against off with a seek and a reset_state() in mid-window; restarts; the
noise -> sample-and-hold -> slew -> filter-cutoff patch.

Holds, pure and exact-sum generators and rectangles are held to the bit.  SlewLimiterPE and the inexact-sum sawtooth
are held to 1e-6 of the case's peak (fixture_harness.PEAK_BOUND): their float64 entry levels / phase sums are re-associated."""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import pygmu2_amd as pg
import control_oracle as P
from control_gpu_common import assert_bits, assert_close, check_case
from fixture_harness import load_cases
from oracle.golden_cases import materialize_array
from pygmu2_amd import look_ahead

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("control")
BY_NAME = {c["name"]: c for c in CASES["cases"]}
FIXED = [c for c in CASES["cases"] if not c.get("fuzz")]
SR = 48000
LONG = 300_000                   # > 131 072: the all-windows slew solve; 147 tiles: several scan segments


@pytest.mark.parametrize("case", FIXED, ids=[c["name"] for c in FIXED])
def test_device_matches_reference(case):
    check_case(case, NPZ)


def started(pe):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    return r


NOISE = materialize_array({"rng": 77, "n": LONG, "ch": 1, "scale": 0.5})


def graphs():
    """name -> (factory of a fresh graph, exact to the bit?)"""
    noise = lambda: pg.ArrayPE(NOISE)                                                    # noqa: E731
    vib = lambda: pg.TransformPE(pg.SinePE(5.0), func=pg.transforms.Affine(20.0, 440.0))  # noqa: E731
    stair = lambda: pg.SampleHoldPE(noise(), pg.PeriodicTrigger(375.0), 0.1)             # noqa: E731
    return {
        "sample_hold": (stair, True),
        "track_hold": (lambda: pg.TrackHoldPE(noise(), pg.PeriodicGate(200.0, 0.3), 0.1), True),
        "slew_linear": (lambda: pg.SlewLimiterPE(stair(), 200.0, 50.0), False),
        "slew_linear_noise": (lambda: pg.SlewLimiterPE(noise(), 2000.0, 5.0), False),
        "slew_exponential": (lambda: pg.SlewLimiterPE(stair(), 2000.0, 100.0, pg.SlewMode.EXPONENTIAL), False),
        "slew_exponential_noise": (lambda: pg.SlewLimiterPE(noise(), 50.0, None, pg.SlewMode.EXPONENTIAL), False),
        "fg_pure_saw": (lambda: pg.FunctionGenPE(441.0, 0.25, 0.1, "sawtooth", 2), True),
        "fg_exact_saw": (lambda: pg.FunctionGenPE(pg.ConstantPE(750.0), 0.25, 0.0, "sawtooth"), True),
        "fg_exact_rect": (lambda: pg.FunctionGenPE(pg.ConstantPE(375.0), pg.ConstantPE(0.375), 0.125, "rectangle", 2), True),
        "fg_vibrato_saw": (lambda: pg.FunctionGenPE(vib(), 0.3, 0.0, "sawtooth"), False),
    }


GRAPHS = graphs()


def spec_of(name):
    """The same graphs as restatement SPECs."""
    noise = {"pe": "ArrayPE", "data": {"rng": 77, "n": LONG, "ch": 1, "scale": 0.5}}
    stair = {"pe": "SampleHoldPE", "source": noise, "trigger": {"pe": "PeriodicTrigger", "hz": 375.0}, "initial_value": 0.1}
    return {
        "sample_hold": stair,
        "track_hold": {"pe": "TrackHoldPE", "source": noise, "initial_value": 0.1,
                       "gate": {"pe": "PeriodicGate", "frequency": 200.0, "duty_cycle": 0.3}},
        "slew_linear": {"pe": "SlewLimiterPE", "source": stair, "rise_rate": 200.0, "fall_rate": 50.0, "mode": "linear"},
        "slew_linear_noise": {"pe": "SlewLimiterPE", "source": noise, "rise_rate": 2000.0, "fall_rate": 5.0, "mode": "linear"},
        "slew_exponential": {"pe": "SlewLimiterPE", "source": stair, "rise_rate": 2000.0, "fall_rate": 100.0,
                             "mode": "exponential"},
        "slew_exponential_noise": {"pe": "SlewLimiterPE", "source": noise, "rise_rate": 50.0, "fall_rate": None,
                                   "mode": "exponential"},
        "fg_exact_saw": {"pe": "FunctionGenPE", "frequency": {"pe": "ConstantPE", "value": 750.0}, "duty_cycle": 0.25,
                         "phase": 0.0, "waveform": "sawtooth"},
    }[name]


def render_blocks(make, sizes, start=0):
    pe = make()
    r = started(pe)
    outs, at = [], start
    for n in sizes:
        outs.append(pe.render(at, n).data.copy())
        at += n
    r.stop()
    return np.concatenate(outs)


def compare(name, got, want, exact):
    (assert_bits if exact else assert_close)(name, got, want)


# ---------------------------------------------------------------------------------------------- long renders
@pytest.mark.parametrize("name", ["sample_hold", "track_hold", "slew_linear", "slew_linear_noise", "slew_exponential",
                                  "slew_exponential_noise", "fg_exact_saw"])
def test_long_render_matches_restatement(name):
    pg.set_sample_rate(SR)
    make, exact = GRAPHS[name]
    got = render_blocks(make, [LONG])
    want, _ = P.run_case({"graph": spec_of(name), "sr": SR, "blocks": [[0, LONG]]})
    compare(f"long_{name}", got, want[0], exact)


def test_long_slew_fallback_gives_the_same_samples(tmp_path):
    """PGX_SLEW_MW_ROUNDS=1: the window-level rounds run out at once and the sequential kernel renders the block."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "slew_long.py"
    script.write_text(textwrap.dedent("""
        import os, sys
        sys.path.insert(0, os.environ["PGX_ROOT"])
        sys.path.insert(0, os.path.join(os.environ["PGX_ROOT"], "tests"))
        import numpy as np
        import pygmu2_amd as pg
        from pygmu2_amd import slew_limiter_pe
        from oracle.golden_cases import materialize_array
        slew_limiter_pe.COUNT_ROUNDS = True
        pg.set_sample_rate(48000)
        x = materialize_array({"rng": 77, "n": 300000, "ch": 1, "scale": 0.5})
        outs, fallbacks = [], 0
        for mode in (pg.SlewMode.LINEAR, pg.SlewMode.EXPONENTIAL):
            pe = pg.SlewLimiterPE(pg.ArrayPE(x), 2000.0, 5.0, mode)
            r = pg.NullRenderer(48000); r.set_source(pe); r.start()
            outs.append(np.concatenate([pe.render(0, 200000).data, pe.render(200000, 100000).data]))
            r.stop()
            fallbacks += pe.stats()["fallbacks"]
        np.save(os.environ["PGX_OUT"], np.concatenate(outs))
        print("FALLBACKS", fallbacks)
    """))
    outs, fallbacks = [], []
    for rounds in ("1", "8"):
        out = str(tmp_path / f"r{rounds}.npy")
        env = dict(os.environ, PGX_ROOT=root, PGX_OUT=out, PGX_SLEW_MW_ROUNDS=rounds)
        p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(np.load(out))
        fallbacks.append(int(p.stdout.split("FALLBACKS")[1].split()[0]))
    # per mode the 200 000-frame render takes the all-windows form, and so does the look-ahead window that the second,
    # contiguous pull opens; with 8 rounds none of them gives up
    assert fallbacks[0] >= 2 and fallbacks[1] == 0
    assert_close("slew_fallback_vs_rounds", outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("sizes", ["1024", "odd"])
def test_streaming_equals_one_big_render(name, sizes):
    pg.set_sample_rate(SR)
    make, exact = GRAPHS[name]
    total = 150 * 1024
    blocks = [1024] * 150 if sizes == "1024" else [997, 1, 2047, 64, 4099, 31] * 21 + [total - 7239 * 21]
    assert sum(blocks) == total
    whole = render_blocks(make, [total], start=-5000)
    parts = render_blocks(make, blocks, start=-5000)
    compare(f"stream_{sizes}_{name}", parts, whole, exact)
    assert float(np.max(np.abs(whole))) > 1e-3               # not silence


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_look_ahead_on_equals_off_with_seek_and_reset(name):
    """40 blocks, a seek, 10 blocks, reset_state() of the top PE in mid-window, 10 blocks."""
    pg.set_sample_rate(SR)
    make, exact = GRAPHS[name]

    def run(flag):
        was = look_ahead.enabled()
        look_ahead.set_enabled(flag)
        try:
            before = look_ahead.STATS["windows"]
            pe = make()
            r = started(pe)
            outs = [pe.render(i * 1024, 1024).data.copy() for i in range(40)]
            outs += [pe.render(102_400 + i * 1024, 1024).data.copy() for i in range(10)]
            pe.reset_state()
            outs += [pe.render(112_640 + i * 1024, 1024).data.copy() for i in range(10)]
            r.stop()
            return np.concatenate(outs), look_ahead.STATS["windows"] - before
        finally:
            look_ahead.set_enabled(was)

    off, windows_off = run(False)
    on, windows_on = run(True)
    assert windows_off == 0
    if not pe_is_pure(make):
        assert windows_on > 0, "the stream was not served from look-ahead windows"
    compare(f"look_ahead_{name}", on, off, exact)


def pe_is_pure(make):
    return make().is_pure()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_restart_reproduces_the_first_run(name):
    pg.set_sample_rate(SR)
    make, _ = GRAPHS[name]
    pe = make()
    r = started(pe)
    first = [pe.render(i * 4096, 4096).data.copy() for i in range(4)]
    r.stop()
    r.start()
    second = [pe.render(i * 4096, 4096).data.copy() for i in range(4)]
    r.stop()
    assert_bits(f"restart_{name}", np.concatenate(second), np.concatenate(first))


def test_non_contiguous_render_carries_hold_and_slew_state():
    pg.set_sample_rate(SR)
    hold = pg.SampleHoldPE(pg.ConstantPE(0.75), pg.ArrayPE(np.array([0, 1, 0, 0], np.float32)), 0.1)
    r = started(hold)
    assert hold.render(0, 4).data[:, 0].tolist() == [np.float32(0.1), 0.75, 0.75, 0.75]
    assert hold.render(1000, 4).data[:, 0].tolist() == [0.75] * 4            # no trigger there: the latch survives
    hold.reset_state()
    assert hold.render(2000, 2).data[:, 0].tolist() == [np.float32(0.1)] * 2
    r.stop()
    slew = pg.SlewLimiterPE(pg.ConstantPE(1.0), 48000.0 / 8)                  # 1/8 per frame
    r = started(slew)
    assert slew.render(0, 4).data[:, 0].tolist() == [0.125, 0.25, 0.375, 0.5]
    assert slew.render(9000, 2).data[:, 0].tolist() == [0.625, 0.75]
    r.stop()
    r.start()
    assert slew.render(0, 1).data[0, 0] == 0.125
    r.stop()


def test_function_gen_restarts_its_phase_on_a_seek():
    pg.set_sample_rate(SR)
    fg = pg.FunctionGenPE(pg.ConstantPE(750.0), 0.0, 0.0, "sawtooth")         # 1/64 cycle per frame
    r = started(fg)
    a = fg.render(0, 100).data.copy()
    b = fg.render(100, 28).data.copy()
    c = fg.render(5000, 100).data.copy()                                      # a seek: from phase 0 again
    r.stop()
    assert_bits("seek", c, a)
    assert a[0, 0] == -1.0 and b[0, 0] == np.float32(2.0 * ((100 % 64) / 64.0) - 1.0)


def test_multichannel_inputs_are_read_in_place():
    """Channel 0 of a stereo source and of a stereo control, without an extraction pass."""
    pg.set_sample_rate(SR)
    rng = np.random.default_rng(5)
    src = rng.standard_normal((5000, 2)).astype(np.float32)
    ctl = (rng.random((5000, 2)) > 0.97).astype(np.float32)
    got = render_blocks(lambda: pg.SampleHoldPE(pg.ArrayPE(src), pg.ArrayPE(ctl), 0.1), [5000])
    want, _ = P.hold_block(0.1, src[:, 0], ctl[:, 0], 0.0)
    assert_bits("stereo_hold", got[:, 0], want)
    got = render_blocks(lambda: pg.SlewLimiterPE(pg.ArrayPE(src), 3000.0), [5000])
    want, _ = P.slew_block(0.0, src[:, 0], 3000.0 / SR, 3000.0 / SR, False)
    assert_close("stereo_slew", got[:, 0], want)


# ---------------------------------------------------------------------------------------------- the patch
def test_sample_hold_slew_filter_patch_against_the_restatement():
    """BiquadPE(BlitSawPE, frequency=affine(SlewLimiterPE(SampleHoldPE(noise, PeriodicTrigger)))), through the public
    names alone."""
    pg.set_sample_rate(SR)
    n = 24000
    x = materialize_array({"rng": 21, "n": n, "ch": 1, "scale": 0.5})
    steps = pg.SampleHoldPE(pg.ArrayPE(x), pg.PeriodicTrigger(12.0))
    glide = pg.SlewLimiterPE(steps, 30.0, 10.0)
    cutoff = pg.TransformPE(glide, func=pg.transforms.Affine(1000.0, 3000.0))
    patch = pg.BiquadPE(pg.BlitSawPE(110.0), frequency=cutoff, q=2.0)
    r = started(patch)
    got = np.concatenate([patch.render(s, 6000).data.copy() for s in range(0, n, 6000)])
    r.stop()
    spec = {"pe": "BiquadPE", "q": 2.0, "source": {"pe": "BlitSawPE", "frequency": 110.0},
            "frequency": {"pe": "TransformPE", "ops": [["affine", 1000.0, 3000.0]],
                          "source": {"pe": "SlewLimiterPE", "rise_rate": 30.0, "fall_rate": 10.0, "mode": "linear",
                                     "source": {"pe": "SampleHoldPE", "initial_value": 0.0,
                                                "source": {"pe": "ArrayPE", "data": {"rng": 21, "n": n, "ch": 1, "scale": 0.5}},
                                                "trigger": {"pe": "PeriodicTrigger", "hz": 12.0}}}}}
    want, _ = P.run_case({"graph": spec, "sr": SR, "blocks": [[s, 6000] for s in range(0, n, 6000)]})
    assert_close("patch_sh_slew_biquad_24000", got, np.concatenate(want))
