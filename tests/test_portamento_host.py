"""CPU: PortamentoPE and ControlPE as far as they go without a device -- validation, repr, properties, purity, the ramp
table the class builds against the numpy restatement of the closed form (tests/portamento_oracle.py), and that
restatement against every block the reference rendered (tests/golden/portamento.npz, tools/gen_golden_portamento.py),
bit for bit: the closed form is pinned to the reference here, the kernel to the closed form in
tests/test_portamento_gpu.py.  The two places where the closed form leaves the reference are asserted against the
zeros the reference rendered there, so they stay visible."""

import numpy as np
import pytest

import fixture_harness as H
import portamento_oracle as PO
import pygmu2_amd as pg

DATA, NPZ = H.load_cases(PO.FIXTURE)
CASES = DATA["cases"]
IDS = [c["name"] for c in CASES]
NOTE = [(60.0, 0, 10)]


@pytest.fixture(autouse=True)
def _sample_rate():
    pg.set_sample_rate(44100)
    yield
    pg.set_sample_rate(44100)


def _blocks(case):
    flat, at = NPZ[case["name"]], 0
    for s, n in case["requests"]:
        yield s, n, flat[at:at + n]
        at += n
    assert at == flat.shape[0]


def test_the_fixture_covers_what_it_should():
    by = {c["name"]: c for c in CASES}
    assert sorted({len(c["notes"]) for c in CASES}) == [1, 2, 3, 4, 5]
    assert {c["channels"] for c in CASES} == {1, 2, 3} and {c["sr"] for c in CASES} == {44100, 48000}
    assert {c["ramp_fraction"] for c in CASES} >= {0.0, 0.3, 1.0} and 0.0 in {c["max_ramp_seconds"] for c in CASES}
    assert by["unsorted"]["notes"] != sorted(by["unsorted"]["notes"], key=lambda n: n[1])
    assert any(n == 1 for c in CASES for _, n in c["requests"])
    for c in CASES:                                             # the generator's own condition, held here too
        if len(c["notes"]) >= 3:
            second = sorted(n[1] for n in c["notes"])[1]
            assert all(s >= second for s, _ in c["requests"]), c["name"]
    # requests that begin exactly at a ramp's at, at + len - 1 and at + len
    at, length, _, _ = PO.case_table(by["two_notes"])
    assert {int(at[0]), int(at[0] + length[0] - 1), int(at[0] + length[0])} <= {s for s, _ in by["two_notes"]["requests"]}
    # a glide that the next note cuts, a ramp of one frame from a note of duration 0, a descending glide
    at, length, v0, v1 = PO.case_table(by["overlap_cut"])
    assert at[0] + length[0] > at[1]
    assert PO.case_table(by["zero_duration"])[1][0] == 1 and by["zero_duration"]["notes"][1][2] == 0
    assert np.all(np.diff([n[0] for n in by["descending"]["notes"]]) < 0)
    assert (PO.case_table(by["max_ramp_binds_44100"])[1].tolist(), PO.case_table(by["max_ramp_binds_48000"])[1].tolist()) \
        == ([441, 441], [480, 480])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_closed_form_reproduces_the_reference_bit_for_bit(case):
    tab = PO.case_table(case)
    for s, n, want in _blocks(case):
        H.assert_bits(f"{case['name']} [{s}, +{n})", PO.line(tab, s, n, case["channels"]), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_class_builds_the_closed_form_s_table(case):
    pg.set_sample_rate(case["sr"])
    pe = PO.build(pg, case)
    want = PO.case_table(case)
    assert len(pe._table) == 4
    for got, col in zip(pe._table, want):
        assert got.dtype == col.dtype and np.array_equal(got, col)
    ref = case["reference"]
    assert repr(pe) == ref["repr"] and pe.is_pure() is ref["pure"] is True and pe.channel_count() == ref["channels"]
    assert [list(n) for n in pe.notes] == ref["notes"]
    ext = pe.extent()
    assert (ext.start, ext.end) == (None, None) and pe.inputs() == []


def test_the_sample_rate_is_read_at_construction():
    notes = [(60.0, 0, 3000), (72.0, 3000, 3000)]
    pg.set_sample_rate(48000)
    pe = pg.PortamentoPE(notes, max_ramp_seconds=0.01)
    pg.set_sample_rate(44100)
    assert pe._table[1].tolist() == [480] and pg.PortamentoPE(notes, max_ramp_seconds=0.01)._table[1].tolist() == [441]


def test_a_fractional_start_is_truncated_after_the_sort():
    pe = pg.PortamentoPE([(60.0, 0, 100), (67.0, 10.9, 100), (64.0, 10.2, 100)])
    assert pe._table[0].tolist() == [10, 10] and pe._table[3].tolist() == [64.0, 67.0]


@pytest.mark.parametrize("d", DATA["departures"], ids=[d["name"] for d in DATA["departures"]])
def test_departures_from_the_reference_are_the_recorded_zeros(d):
    """Where the reference renders 0 (a request before the second of three notes; before two notes that share a start),
    the closed form holds the first pitch, as the reference's docstring says; every other frame agrees to the bit."""
    ref = NPZ[f"departure/{d['name']}"]
    s, n = d["request"]
    a, b = d["zero_frames"]
    want = PO.line(PO.case_table(d), s, n)
    first_pitch = sorted(d["notes"], key=lambda x: x[1])[0][0]
    assert ref.shape == want.shape == (n, 1)
    assert not np.any(ref[a:b]) and np.all(want[a:b] == np.float32(first_pitch))
    keep = np.ones(n, bool)
    keep[a:b] = False
    H.assert_bits(d["name"], want[keep], ref[keep])
    assert (b > a) == (d["name"] != "straddling_second_note")


def test_validation_messages_are_the_reference_s():
    errors = DATA["errors"]
    refusals = {"empty": lambda: pg.PortamentoPE([]),
                "negative_max_ramp": lambda: pg.PortamentoPE(NOTE, max_ramp_seconds=-0.5),
                "fraction_above_1": lambda: pg.PortamentoPE(NOTE, ramp_fraction=1.5),
                "fraction_below_0": lambda: pg.PortamentoPE(NOTE, ramp_fraction=-0.25),
                "no_channels": lambda: pg.PortamentoPE(NOTE, channels=0)}
    assert sorted(refusals) == sorted(errors)
    for key, make in refusals.items():
        with pytest.raises(ValueError) as e:
            make()
        assert str(e.value) == errors[key], key


def test_repr_and_properties():
    notes = [(73.0, 1000, 1000), (69.0, 0, 1000), (76.0, 2000, 1000)]
    pe = pg.PortamentoPE(notes)
    assert repr(pe) == "PortamentoPE(3 notes, max_ramp_seconds=0.1, ramp_fraction=0.3, channels=1)"
    assert pe.notes == sorted(notes, key=lambda n: n[1]) and pe.notes is not pe.notes
    assert (pe.max_ramp_seconds, pe.ramp_fraction, pe.channel_count()) == (0.1, 0.3, 1)
    assert pe.is_pure() and pe._READ_AHEAD_SAFE is True
    pe.notes.append((0.0, 0, 0))                                # a copy: the PE keeps its own
    assert len(pe.notes) == 3


def test_control_pe_on_the_host():
    c = pg.ControlPE()
    assert (c.value, c.channel_count(), c.is_pure(), c.inputs()) == (0.0, 1, False, [])
    assert repr(c) == "ControlPE(value=0.0, channels=1)" and repr(pg.ControlPE(1.5, channels=2)) == "ControlPE(value=1.5, channels=2)"
    ext = c.extent()
    assert (ext.start, ext.end) == (None, None)
    c.set_value(3.0)
    assert c.value == 0.0                                       # only a render consumes the queue
    assert not getattr(pg.ControlPE, "_READ_AHEAD_SAFE", False) and not getattr(pg.ControlPE, "_LOOK_AHEAD_SAFE", False)
    from pygmu2_amd import look_ahead, read_ahead
    warp = pg.TimeWarpPE(pg.SinePE(220.0), rate=c)
    assert not read_ahead.eligible(c) and not read_ahead.eligible(warp) and not look_ahead.capable(warp)
    gain = pg.GainPE(pg.SinePE(220.0), c)                       # GainPE and SinePE take part in windows, ControlPE vetoes
    assert not read_ahead.eligible(gain) and not look_ahead.capable(gain)


def test_bound_in_the_package_and_not_in_all():
    from pygmu2_amd.control_pe import ControlPE
    from pygmu2_amd.portamento_pe import PortamentoPE
    assert pg.PortamentoPE is PortamentoPE and pg.ControlPE is ControlPE
    assert "PortamentoPE" not in pg.__all__ and "ControlPE" not in pg.__all__
