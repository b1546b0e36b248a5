"""GPU: WavetablePE / TimeWarpPE on the device against the reference-rendered fixtures (tests/golden/playback.npz):
every mode x interpolation, tables and sources of every kind of extent, block sizes 1 .. 48000, lifecycle calls and
gaps; streaming in small blocks; the kept table and the scalar-rate window cost no device-to-host copy; the graphs
of the reference's example 20."""

import numpy as np
import pytest

import pygmu2_amd as pg
import playback_oracle as P
from oracle.golden_cases import materialize_array
from fixture_harness import PEAK_BOUND, bits_equal, load_cases, split_blocks
from playback_gpu_common import build_case, check_case
from pygmu2_amd import diagnostics, timewarp_pe, wavetable_pe

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("playback")
BY_NAME = {c["name"]: c for c in CASES["cases"]}
FIXED = [c for c in CASES["cases"] if not c.get("fuzz")]
SR = 48000


@pytest.mark.parametrize("case", FIXED, ids=[c["name"] for c in FIXED])
def test_device_matches_reference(case):
    check_case(case, NPZ)


def started(pe):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    return r


def sine_table(n=2048):
    return pg.ArrayPE(np.sin(2 * np.pi * np.arange(n) / n).astype(np.float32))


def saw_index(n=2048):
    return pg.LoopPE(pg.PiecewisePE([(0, 0.0), (109, float(n))]), 0, 109)


# ---------------------------------------------------------------------------------------------- streaming
def test_wavetable_small_blocks_equal_one_large_render():
    pg.set_sample_rate(SR)
    make = lambda: pg.WavetablePE(sine_table(), saw_index(), pg.InterpolationMode.CUBIC, pg.OutOfBoundsMode.WRAP)  # noqa: E731
    whole_pe = make()
    r = started(whole_pe)
    whole = whole_pe.render(0, 64 * 100).data.copy()
    r.stop()
    pe = make()
    r = started(pe)
    parts = [pe.render(i * 64, 64).data.copy() for i in range(100)]
    r.stop()
    assert bits_equal(np.concatenate(parts), whole)
    assert float(np.max(np.abs(whole))) > 0.9


def test_timewarp_small_blocks_equal_fixture_blocks():
    case = BY_NAME["tw_stream_64"]
    assert all(n == 64 for _, n in case["blocks"]) and case["compare"] == "bits"
    check_case(case, NPZ)


@pytest.mark.parametrize("name", ["tw_reset_scalar", "tw_reset_pe_rate"])
def test_reset_and_restart_rewind_the_head(name):
    case = BY_NAME[name]
    assert case["ops"] == {"2": "reset", "4": "restart"}
    check_case(case, NPZ)
    # the fixture shows the head back at 0: the blocks after each call repeat the first two
    blocks = split_blocks(case, NPZ[name])
    assert bits_equal(blocks[2], blocks[0]) and bits_equal(blocks[4], blocks[0]) and bits_equal(blocks[5], blocks[1])


# ---------------------------------------------------------------------------------------------- no read-back
def pulls_of(pe):
    return diagnostics.report()["pulls"].get(f"{type(pe).__name__}@{id(pe):x}", 0)


def test_kept_table_and_scalar_rate_issue_no_device_to_host_copy():
    pg.set_sample_rate(SR)
    table = sine_table()
    osc = pg.WavetablePE(table, saw_index(), pg.InterpolationMode.CUBIC, pg.OutOfBoundsMode.WRAP)
    tape_src = pg.ArrayPE(materialize_array({"rng": 5, "n": 30000}))
    tape = pg.TimeWarpPE(tape_src, 1.5, pg.InterpolationMode.CUBIC)
    diagnostics.reset()
    diagnostics.enable(pull_counts=True, timing=False)
    try:
        for pe in (osc, tape):
            r = started(pe)
            for i in range(100):
                pe.render(i * 128, 128)
            r.stop()
        assert pulls_of(table) == 1                  # rendered once, kept in HBM
        assert pulls_of(osc) == 100 and pulls_of(tape) == 100 and pulls_of(tape_src) == 100
        assert osc.d2h_reads == 0 and tape.d2h_reads == 0
    finally:
        diagnostics.disable()
        diagnostics.reset()


def test_data_dependent_windows_read_sixteen_bytes_per_render():
    pg.set_sample_rate(SR)
    index = pg.TransformPE(pg.SinePE(31.0), func=pg.transforms.Affine(3000.0, 0.0))
    unbounded = pg.WavetablePE(pg.SinePE(100.0), index)                           # no extent to keep
    ramp = pg.TimeWarpPE(pg.SinePE(220.0), pg.PiecewisePE([(0, 2.0), (4096, -2.0)]))
    for pe in (unbounded, ramp):
        r = started(pe)
        for i in range(10):
            pe.render(i * 256, 256)
        r.stop()
        assert pe.d2h_reads == 10


def test_switched_off_paths_give_the_same_samples(monkeypatch):
    """KEEP_TABLE / NO_READBACK only choose how the window is found (what tools/playback_probe.py measures)."""
    for name in ("wt_wrap_cubic", "wt_offset_zero_linear", "wt_stereo_wrap_cubic", "tw_rate_1.5_cubic", "tw_rate_-1_linear"):
        check_case(BY_NAME[name], NPZ)
    monkeypatch.setattr(wavetable_pe, "KEEP_TABLE", False)
    monkeypatch.setattr(timewarp_pe, "NO_READBACK", False)
    for name in ("wt_wrap_cubic", "wt_offset_zero_linear", "wt_stereo_wrap_cubic", "tw_rate_1.5_cubic", "tw_rate_-1_linear"):
        check_case(BY_NAME[name], NPZ)
    pe, made = build_case(BY_NAME["wt_wrap_cubic"])
    r = started(pe)
    pe.render(0, 64)
    pe.render(64, 64)
    r.stop()
    assert made[0].d2h_reads == 2


def test_kept_table_is_dropped_on_start_and_stop():
    pg.set_sample_rate(SR)
    osc = pg.WavetablePE(sine_table(256), saw_index(256))
    r = started(osc)
    osc.render(0, 64)
    assert osc._kept is not None
    r.stop()
    assert osc._kept is None
    r.start()
    assert osc._kept is None
    r.stop()


def test_very_large_table_is_not_kept(monkeypatch):
    monkeypatch.setattr(wavetable_pe, "KEPT_TABLE_MAX_BYTES", 1024)
    check_case(BY_NAME["wt_clamp_cubic"], NPZ)
    pe, made = build_case(BY_NAME["wt_clamp_cubic"])
    r = started(pe)
    pe.render(0, 64)
    r.stop()
    assert made[0]._kept is None and made[0].d2h_reads == 1


def test_non_finite_positions_raise():
    pg.set_sample_rate(SR)
    with pytest.raises(ValueError, match="not finite"):
        pg.TimeWarpPE(pg.SinePE(220.0), pg.ConstantPE(float("inf"))).render(0, 64)
    with pytest.raises(ValueError, match="not finite"):
        pg.TimeWarpPE(pg.SinePE(220.0), float("nan")).render(0, 64)
    with pytest.raises(ValueError, match="non-finite"):
        pg.WavetablePE(pg.SinePE(100.0), pg.ConstantPE(float("nan"))).render(0, 64)
    # one NaN at frame 0 of a block longer than the range kernels' thread stride: frames 256 and 512 follow it
    stream = np.linspace(1.0, 40.0, 600, dtype=np.float32)
    stream[0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        pg.DelayPE(pg.SinePE(220.0), delay=pg.ArrayPE(stream)).render(0, 600)
    with pytest.raises(ValueError, match="non-finite"):
        pg.WavetablePE(pg.SinePE(100.0), pg.ArrayPE(stream)).render(0, 600)


# ---------------------------------------------------------------------------------------------- example 20
def example20(rate_points, n):
    pg.set_sample_rate(SR)
    buf = materialize_array({"rng": 7, "n": 6000, "ch": 1, "scale": 0.5})
    warped = pg.TimeWarpPE(pg.LoopPE(pg.ArrayPE(buf), crossfade_seconds=0.01), rate=pg.PiecewisePE(rate_points))
    return pg.CropPE(pg.GainPE(warped, 0.8), 0, n)


def test_example20_speed_ramp():
    case = BY_NAME["ex20_speed_ramp"]
    n = 24000
    pe = example20([(0, 0.25), (n, 5.0)], n)
    r = started(pe)
    outs = [pe.render(int(s), int(c)).data.copy() for s, c in case["blocks"]]
    r.stop()
    for i, want in split_blocks(case, NPZ[case["name"]]).items():
        assert bits_equal(outs[i], want), f"block {i}"
    assert float(np.max(np.abs(NPZ[case["name"]]))) > 0.5


def test_example20_jog_shuttle():
    case = BY_NAME["ex20_jog_shuttle_48000"]
    pe = example20([(0, 2.0), (48000, -2.0)], 48000)
    r = started(pe)
    out = pe.render(0, 48000).data.copy()
    r.stop()
    assert bits_equal(out, NPZ[case["name"]])


def test_wavetable_oscillator_under_a_tape_head():
    """A 2048-frame sine table read by a ~440 Hz saw, then played forwards and backwards by a rate ramp 2 -> -2: the
    device against the restatement, through the public names alone."""
    pg.set_sample_rate(SR)
    table = pg.ArrayPE(np.sin(2 * np.pi * np.arange(2048) / 2048).astype(np.float32))
    saw = pg.LoopPE(pg.PiecewisePE([(0, 0.0), (109, 2048.0)]), 0, 109)
    osc = pg.WavetablePE(table, saw, pg.InterpolationMode.CUBIC, pg.OutOfBoundsMode.WRAP)
    tape = pg.TimeWarpPE(pg.CropPE(osc, 0, 96000), rate=pg.PiecewisePE([(0, 2.0), (48000, -2.0)]))
    r = started(tape)
    got = [tape.render(s, 12000).data.copy() for s in range(0, 48000, 12000)]
    r.stop()
    values = np.sin(2 * np.pi * np.arange(2048) / 2048).astype(np.float32)
    spec = {"pe": "TimeWarpPE", "rate": {"pe": "PiecewisePE", "points": [[0, 2.0], [48000, -2.0]]},
            "source": {"pe": "CropPE", "start": 0, "duration": 96000,
                       "source": {"pe": "WavetablePE", "interpolation": "cubic", "out_of_bounds": "wrap",
                                  "wavetable": {"pe": "ArrayPE", "data": {"values": values.tolist()}},
                                  "indexer": {"pe": "LoopPE", "loop_start": 0, "loop_end": 109,
                                              "source": {"pe": "PiecewisePE", "points": [[0, 0.0], [109, 2048.0]]}}}}}
    want, _ = P.run_case({"graph": spec, "sr": SR, "blocks": [[s, 12000] for s in range(0, 48000, 12000)]})
    got, want = np.concatenate(got), np.concatenate(want)
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    print(f"PLAYBACK_ERR oscillator_under_tape max_abs_err={err:.3e} peak={peak:.3e}")
    assert peak > 0.9 and err <= PEAK_BOUND * peak
