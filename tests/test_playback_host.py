"""CPU: WavetablePE / TimeWarpPE without a device.  The numpy restatement (tests/playback_oracle.py) reproduces every
stored block of the reference-rendered fixtures bit for bit; the classes' host side -- extents, repr, inputs(), purity,
channel counts, export, errors -- is the reference's as the fixtures recorded it."""

import numpy as np
import pytest

import pygmu2_amd as pg
import playback_oracle as P
import spec_build
from fixture_harness import bits_equal, load_cases, split_blocks

CASES, NPZ = load_cases("playback")
ALL = CASES["cases"]


def build_pg(case):
    return spec_build.build_case(case, P.NEW_KINDS)


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_restatement_equals_fixture_bit_for_bit(case):
    outs, _ = P.run_case(case)
    stored = split_blocks(case, NPZ[case["name"]])
    assert stored
    for i, want in stored.items():
        assert bits_equal(outs[i], want), f"{case['name']}: block {i} differs"


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_host_side_matches_reference(case):
    pe, made = build_pg(case)
    ext = pe.extent()
    assert [ext.start, ext.end] == case["extent"]
    assert len(made) == len(case["new_pes"]) > 0
    for m, ref in zip(made, case["new_pes"]):
        assert repr(m) == ref["repr"]
        assert [m.extent().start, m.extent().end] == ref["extent"]
        assert m.is_pure() is ref["pure"]
        assert m.channel_count() == ref["channels"]
        assert [type(i).__name__ for i in m.inputs()] == ref["inputs"]
    # the restatement's extent arithmetic agrees as well
    root = P.PlaybackNode(case["graph"], case["sr"])
    assert list(root.extent()) == case["extent"]


def test_fixture_covers_what_it_must():
    names = {c["name"] for c in ALL}
    for mode in ("zero", "clamp", "wrap"):
        for interp in ("linear", "cubic"):
            assert f"wt_{mode}_{interp}" in names and f"wt_offset_{mode}_{interp}" in names
        assert f"wt_unbounded_{mode}" in names
    for rate in ("1", "1.5", "0.25", "-1", "0", "1.1"):
        assert f"tw_rate_{rate}_linear" in names
    sizes = {int(n) for c in ALL for _, n in c["blocks"]}
    assert {1, 64, 1024, 48000} <= sizes
    assert sum(1 for c in ALL if c.get("fuzz")) >= 40
    assert {c["compare"] for c in ALL} == {"bits", "peak"}
    # every graph whose head positions are exact sums is held to the bit: only float64 rates such as 1.1 are not
    assert all(c["compare"] == "bits" for c in ALL if c["name"].startswith("wt_"))


def test_timewarp_scalar_extent_branches():
    pg.set_sample_rate(48000)
    src = pg.DelayPE(pg.ArrayPE(np.zeros(3000, np.float32)), -1500)                  # extent [-1500, 1500)
    ext = lambda r, s=src: (lambda e: (e.start, e.end))(pg.TimeWarpPE(s, r).extent())   # noqa: E731
    assert ext(0.0) == (None, None)                                                  # the head stands inside for ever
    assert ext(0.0, pg.DelayPE(pg.ArrayPE(np.zeros(10, np.float32)), 5)) == (0, 0)   # ... or outside for ever
    assert ext(1.5) == (0, 1000)
    assert ext(0.25) == (0, 6000)
    assert ext(-1.0) == (0, 1501)
    late = pg.DelayPE(pg.ArrayPE(np.zeros(2000, np.float32)), 500)                   # extent [500, 2500)
    assert ext(2.0, late) == (250, 1250)
    assert ext(-1.0, late) == (0, 0)
    assert ext(1.0, pg.SinePE(220.0)) == (None, None)
    rate = pg.PiecewisePE([(100, 1.0), (900, 2.0)])
    assert pg.TimeWarpPE(src, rate).extent() == rate.extent()
    for r in (1.5, 0.25, -1.0, 0.0):
        assert (lambda e: (e.start, e.end))(pg.TimeWarpPE(src, r).extent()) == P.timewarp_extent((-1500, 1500), r)


def test_export_and_properties():
    assert pg.WavetablePE.__name__ == "WavetablePE" and pg.TimeWarpPE.__name__ == "TimeWarpPE"
    # bound in the namespace, not in __all__: entering the fuzz census of exported PEs is a later change
    assert "WavetablePE" not in pg.__all__ and "TimeWarpPE" not in pg.__all__
    assert [m.value for m in pg.OutOfBoundsMode] == ["zero", "clamp", "wrap"]
    from pygmu2_amd import delay_pe, timewarp_pe, wavetable_pe
    assert wavetable_pe.InterpolationMode is delay_pe.InterpolationMode is timewarp_pe.InterpolationMode
    pg.set_sample_rate(48000)
    table, index = pg.ArrayPE(np.zeros(16, np.float32)), pg.SinePE(1.0)
    wt = pg.WavetablePE(table, index)
    assert wt.wavetable is table and wt.indexer is index
    assert wt.interpolation is pg.InterpolationMode.LINEAR and wt.out_of_bounds is pg.OutOfBoundsMode.ZERO
    assert wt.is_pure() and wt.d2h_reads == 0
    tw = pg.TimeWarpPE(table)
    assert tw.source is table and tw.rate == 1.0 and tw.interpolation is pg.InterpolationMode.LINEAR
    assert not tw.is_pure() and tw.inputs() == [table]
    assert not getattr(tw, "_LOOK_AHEAD_SAFE", False) and not getattr(tw, "_READ_AHEAD_SAFE", False)
    assert repr(pg.TimeWarpPE(table, index)) == "TimeWarpPE(source=ArrayPE, rate=SinePE(...), interpolation=linear)"


def test_errors_follow_the_conventions():
    pg.set_sample_rate(48000)
    table = pg.ArrayPE(np.zeros(16, np.float32))
    for pe in (pg.WavetablePE(table, pg.SinePE(1.0)), pg.TimeWarpPE(table, 1.5)):
        with pytest.raises(ValueError, match="duration must be >= 0"):
            pe.render(0, -1)
        empty = pe.render(7, 0)                                   # no kernel, no device needed
        assert empty.start == 7 and empty.duration == 0 and empty.channels == 1
