"""CPU: the temperament classes, the global tuning and the four tuning conversions against what the reference recorded
(tests/golden/tuning_cases.json, tuning.npz), how transforms.lower() and the tuning descriptors treat them, and the C
layout of pgx_tuning's structs.  Nothing here touches the device."""

import functools
import warnings

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, temperament, transforms
from fixture_harness import load_cases
import tuning_oracle as T

DATA, NPZ = load_cases("tuning")
M = T.package_namespace()


@pytest.fixture(autouse=True)
def _default_tuning():
    T.default_tuning(pg)
    yield
    T.default_tuning(pg)


# ---------------------------------------------------------------------------------------------- the reference's records
@pytest.mark.parametrize("index", range(len(DATA["functions"])),
                         ids=lambda i: "{temperament_name}-{fn}-{input}".format(**DATA["functions"][i]) + f"-{i}")
def test_function_records_within_an_ulp(index):
    rec = DATA["functions"][index]
    want = NPZ[f"fn/{index}"]
    got = np.asarray(T.call_function(M, rec, DATA["inputs"][rec["input"]]))
    assert got.dtype == np.float64 and got.shape == want.shape
    # 2.0 ** and log2 go through libm, whose last bit may differ between builds: within 1 ulp
    if rec["fn"] == "freq_to_pitch":
        scale = np.spacing(128.0)                                # an ulp of the sum's size
    elif rec["fn"] == "ratio_to_semitones":
        scale = np.spacing(np.maximum(np.abs(want), 1.0))
    else:
        scale = np.spacing(np.abs(want))
    assert np.max(np.abs(got - want) / scale) <= 1


@pytest.mark.parametrize("name", sorted(T_ for T_ in DATA["temperaments"] if not T_.startswith("custom")))
def test_shapes_names_and_reprs(name):
    want = DATA["temperaments"][name]
    spec = next(r["temperament"] for r in DATA["functions"] if r["temperament_name"] == name)
    t = T.temperament(pg, spec)
    assert isinstance(t, pg.Temperament)
    assert t.name() == want["name"] and repr(t) == want["repr"]
    assert getattr(t, "num_notes", None) == want["num_notes"] and getattr(t, "divisions", None) == want["divisions"]
    for fn, scalar in (("pitch_to_freq", 60), ("freq_to_pitch", 300.0), ("interval_to_ratio", 7),
                       ("ratio_to_interval", 1.4)):
        assert T.shape_of(getattr(t, fn), scalar) == want["shapes"][fn]["scalar"], fn
        assert T.shape_of(getattr(t, fn), [scalar, scalar * 1.01]) == want["shapes"][fn]["list"], fn


def test_scalar_shapes_differ_between_equal_and_just():
    assert np.shape(pg.EqualTemperament().pitch_to_freq(60)) == ()
    assert np.shape(pg.JustIntonation().pitch_to_freq(60)) == (1,)
    assert np.shape(pg.pitch_to_freq(60, temperament=pg.PythagoreanTuning())) == (1,)


def test_ratios_is_a_copy():
    ji = pg.JustIntonation()
    r = ji.ratios
    r[0] = 7.0
    assert ji.ratios[0] == 1.0 and ji.num_notes == 12 and ji.ratios.dtype == np.float64


def test_validation_errors_are_the_reference_s():
    refusals = {"divisions_zero": lambda: pg.EqualTemperament(0),
                "one_ratio": lambda: pg.JustIntonation([1.0]),
                "no_unison": lambda: pg.JustIntonation([1.1, 1.5]),
                "reference_zero": lambda: pg.set_reference_frequency(0.0),
                "reference_negative": lambda: pg.set_reference_frequency(-440.0, 60.0)}
    assert sorted(refusals) == sorted(DATA["errors"])
    for key, make in refusals.items():
        with pytest.raises(ValueError) as info:
            make()
        assert str(info.value) == DATA["errors"][key]["text"], key
    assert pg.get_reference_frequency() == (440.0, 69.0)          # a refused value leaves the globals alone


def test_custom_temperament_passes_through():
    calls = []

    def p2f(p, ref_pitch, ref_freq):
        calls.append((ref_pitch, ref_freq))
        return ref_freq * 2.001 ** ((np.asarray(p) - ref_pitch) / 12)
    custom = pg.CustomTemperament(p2f, lambda f, rp, rf: [1, 2], lambda i: 3, lambda r: 4.5, name="Stretched")
    assert custom.name() == DATA["temperaments"]["custom"]["name"] and repr(custom) == DATA["temperaments"]["custom"]["repr"]
    assert pg.CustomTemperament(None, None, None, None).name() == DATA["temperaments"]["custom_default"]["name"]
    got = pg.pitch_to_freq([69, 81], temperament=custom, reference_freq=432.0)
    assert calls == [(69.0, 432.0)] and got.dtype == np.float64 and got.tolist() == [432.0, 432.0 * 2.001]
    assert pg.freq_to_pitch(1.0, temperament=custom).tolist() == [1.0, 2.0]
    assert pg.semitones_to_ratio(0, temperament=custom) == 3.0 and pg.ratio_to_semitones(0, temperament=custom) == 4.5


# ---------------------------------------------------------------------------------------------- the globals
def test_globals_round_trip():
    assert repr(pg.get_temperament()) == DATA["initial_temperament"]
    assert list(pg.get_reference_frequency()) == DATA["helpers"]["initial"]
    for helper in ("set_verdi_tuning", "set_baroque_pitch", "set_concert_pitch"):
        getattr(pg, helper)()
        assert list(pg.get_reference_frequency()) == DATA["helpers"][helper], helper
    pg.set_reference_frequency(442, 57)
    assert [repr(v) for v in pg.get_reference_frequency()] == DATA["helpers"]["set_reference_frequency(442, 57)"]
    before = temperament.epoch()
    ji = pg.JustIntonation()
    pg.set_temperament(ji)
    assert pg.get_temperament() is ji and temperament.epoch() == before + 1
    pg.set_verdi_tuning()
    assert temperament.epoch() == before + 2


def test_conversions_resolve_the_globals_when_called():
    assert pg.pitch_to_freq(69) == 440.0
    pg.set_verdi_tuning()
    assert pg.pitch_to_freq(69) == 432.0 and pg.freq_to_pitch(432.0) == 69.0
    assert pg.pitch_to_freq(69, reference_freq=415.0) == 415.0
    assert pg.pitch_to_freq(60, reference_pitch=60.0) == 432.0
    pg.set_temperament(pg.EqualTemperament(19))
    assert pg.semitones_to_ratio(19) == 2.0 and pg.ratio_to_semitones(2.0) == 19.0
    assert pg.semitones_to_ratio(12, temperament=pg.EqualTemperament(12)) == 2.0
    pg.set_temperament(pg.JustIntonation())
    assert pg.semitones_to_ratio([7.0]).tolist() == [1.5]


def test_anything_but_a_temperament_is_refused():
    with pytest.raises(NotImplementedError, match="temperament.*EqualTemperament"):
        pg.pitch_to_freq(60.0, temperament="just")


def test_new_names_are_bound_and_not_exported():
    for name in ("Temperament", "EqualTemperament", "JustIntonation", "PythagoreanTuning", "CustomTemperament",
                 "set_temperament", "get_temperament", "set_reference_frequency", "get_reference_frequency",
                 "set_concert_pitch", "set_verdi_tuning", "set_baroque_pitch", "temperament"):
        assert hasattr(pg, name), name
        assert name not in pg.__all__, name


# ---------------------------------------------------------------------------------------------- the quirks
def test_scale_degree_rounds_to_n_and_the_frequency_halves():
    ji = pg.JustIntonation(reference_pitch=0.0)
    rel = -5e-16                                                 # floor(rel / 12) = -1, and rel + 12 rounds to exactly 12.0
    assert rel - np.floor(rel / 12) * 12 == 12.0
    unison = ji.pitch_to_freq(0.0)[0]
    assert ji.pitch_to_freq(rel)[0] == unison / 2                # index 12 % 12 == 0 in the LOWER octave
    assert abs(ji.pitch_to_freq(-1e-9)[0] / unison - 1.0) < 1e-9  # a little further down it is the unison's neighbour
    assert ji.interval_to_ratio(rel)[0] == 0.5 and ji.interval_to_ratio(0.0)[0] == 1.0


def test_just_interpolation_doubles_the_ratio_across_the_octave():
    ji = pg.JustIntonation([1.0, 1.5], reference_pitch=57.0)
    assert ji.interval_to_ratio([0.0, 1.0, 2.0, 3.0, -1.0]).tolist() == [1.0, 1.5, 2.0, 3.0, 0.75]
    half = ji.interval_to_ratio(1.5)[0]                          # between 3/2 and 2/1, geometric
    assert half == 2.0 ** (np.log2(1.5) + 0.5 * (np.log2(2.0) - np.log2(1.5)))


def test_just_inverse_is_the_nearest_entry_first_minimum_and_floored():
    ji = pg.JustIntonation([1.0, 1.25, 1.5], reference_pitch=0.0)
    assert ji.ratio_to_interval([1.0, 1.2, 1.4, 1.9, 2.6]).tolist() == [0.0, 1.0, 2.0, 2.0, 4.0]
    assert ji.ratio_to_interval([1.125]).tolist() == [0.0]        # |1 - 1.125| == |1.25 - 1.125|: the first
    assert ji.ratio_to_interval([0.0]).tolist() == ji.ratio_to_interval([1e-10]).tolist()
    assert ji.ratio_to_interval([-5.0]).tolist() == ji.ratio_to_interval([1e-10]).tolist()


# ---------------------------------------------------------------------------------------------- lowering
CONVERSIONS = {"pitch_to_freq": transforms.PitchToFreq, "freq_to_pitch": transforms.FreqToPitch,
               "semitones_to_ratio": transforms.SemitonesToRatio, "ratio_to_semitones": transforms.RatioToSemitones}


@pytest.mark.parametrize("name", sorted(CONVERSIONS))
def test_lower_recognises_the_function_and_keyword_partials(name):
    fn = getattr(pg, name)
    got = transforms.lower(fn)
    assert type(got) is CONVERSIONS[name] and got.temperament is None and got.follows_globals()
    ji = pg.JustIntonation()
    got = transforms.lower(functools.partial(fn, temperament=ji))
    assert type(got) is CONVERSIONS[name] and got.temperament is ji
    assert got.follows_globals() == (name in ("pitch_to_freq", "freq_to_pitch"))     # the reference is still the global one
    if name in ("pitch_to_freq", "freq_to_pitch"):
        got = transforms.lower(functools.partial(fn, temperament=ji, reference_pitch=60, reference_freq=256.0))
        assert (got.reference_pitch, got.reference_freq) == (60.0, 256.0) and not got.follows_globals()
    # a positional argument, a lambda, a keyword the function does not take, host code: opaque host callables
    assert transforms.lower(functools.partial(fn, 60.0)) is None
    assert transforms.lower(lambda v: fn(v)) is None
    assert transforms.lower(functools.partial(fn, tuning=ji)) is None
    custom = pg.CustomTemperament(None, None, None, None)
    assert transforms.lower(functools.partial(fn, temperament=custom)) is None
    assert transforms.lower(CONVERSIONS[name](custom)) is None
    assert transforms.lower(transforms.Chain(transforms.Abs(), CONVERSIONS[name](custom))) is None


@pytest.mark.parametrize("name", sorted(CONVERSIONS))
def test_descriptor_call_is_the_conversions_function(name):
    x = np.array([[0.7, 61.3], [440.0, 3.1]])
    kinds = [None, pg.EqualTemperament(19), pg.PythagoreanTuning()]
    if name in ("freq_to_pitch", "ratio_to_semitones"):
        x, kinds = x[:, :1], kinds                               # the just inverse takes rows of one sample
    for t in kinds:
        kw = {"temperament": t}
        if name in ("pitch_to_freq", "freq_to_pitch"):
            kw.update(reference_pitch=60.0, reference_freq=256.0)
        want = getattr(pg, name)(x, **kw)
        got = CONVERSIONS[name](**kw)(x)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    pg.set_temperament(pg.JustIntonation())
    pg.set_baroque_pitch()
    assert np.array_equal(CONVERSIONS[name]()(x), getattr(pg, name)(x))      # None: the globals, at call time


def test_chain_lists_its_ops_in_order():
    chain = transforms.Chain(transforms.Affine(12.0, 60.0), transforms.PitchToFreq(), transforms.Clip(200.0, 400.0))
    ops = chain.ops()
    assert [op[0] for op in ops] == [transforms.AFFINE, transforms.ET_PITCH_TO_FREQ, transforms.CLIP]
    assert ops[0][1:] == (12.0, 60.0) and ops[2][1:] == (200.0, 400.0)
    assert ops[1][1] == temperament.DeviceTuning(False, 69.0, 440.0, 12.0, None)
    assert chain.follows_globals() and chain.lowerable()
    pg.set_temperament(pg.JustIntonation([1.0, 1.5], reference_pitch=57.0))
    pg.set_reference_frequency(432.0, 57.0)
    code, tuning, _ = chain.ops()[1]
    assert code == transforms.JI_PITCH_TO_FREQ and tuning.just and tuning.divisions == 2.0
    assert (tuning.reference_pitch, tuning.reference_freq) == (57.0, 432.0)
    assert tuning.table.tolist() == [0.0, np.log2(1.5), 1.0, 1.0, 1.5]          # N + 1 logarithms, then the N ratios
    pg.set_temperament(pg.CustomTemperament(None, None, None, None))
    with pytest.raises(LookupError):
        chain.ops()
    # interval <-> ratio: reference pitch 0 and frequency 1
    code, tuning, _ = transforms.RatioToSemitones(pg.EqualTemperament(19)).ops()[0]
    assert code == transforms.ET_FREQ_TO_PITCH and tuning[1:4] == (0.0, 1.0, 19.0)


def test_from_spec_builds_the_tuning_steps():
    chain = transforms.from_spec([["affine", 2.0, 1.0],
                                  ["pitch_to_freq", {"kind": "just", "ratios": [1.0, 1.25, 1.5], "reference_pitch": 57.0}, 69.0, 440.0],
                                  ["ratio_to_semitones", {"kind": "equal", "divisions": 19}], ["freq_to_pitch", None]])
    a, b, c = chain.steps[1:]
    assert type(a) is transforms.PitchToFreq and a.temperament.num_notes == 3 and not a.follows_globals()
    assert type(b) is transforms.RatioToSemitones and b.temperament.divisions == 19
    assert type(c) is transforms.FreqToPitch and c.temperament is None and c.follows_globals()
    assert isinstance(transforms.temperament_from_spec({"kind": "pythagorean"}), pg.PythagoreanTuning)


def test_read_ahead_only_with_everything_explicit():
    """a step that follows the globals is read when a block is rendered, so its TransformPE opens no window."""
    src = pg.ConstantPE(60.0)
    assert pg.TransformPE(src, func=pg.pitch_to_freq)._read_ahead_condition() is False
    assert pg.TransformPE(src, func=transforms.PitchToFreq(pg.JustIntonation()))._read_ahead_condition() is False
    explicit = transforms.PitchToFreq(pg.JustIntonation(), 69.0, 440.0)
    assert pg.TransformPE(src, func=explicit)._read_ahead_condition() is True
    assert pg.TransformPE(src, func=transforms.SemitonesToRatio(pg.EqualTemperament()))._read_ahead_condition() is True
    assert pg.TransformPE(src, func=transforms.Abs())._read_ahead_condition() is True
    assert pg.TransformPE(src, func=lambda v: v)._read_ahead_condition() is False


def test_a_size_one_array_is_a_scalar_parameter():
    freq = pg.pitch_to_freq(60, temperament=pg.JustIntonation())                  # example 20's line: shape (1,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sine = pg.SinePE(frequency=freq, amplitude=np.array([0.2]))
        assert type(sine.frequency) is float and sine.frequency == float(freq[0]) and sine.amplitude == 0.2
        assert sine.is_pure() and "frequency=264.0" in repr(sine)
    assert pg.SinePE(440.0).frequency == 440.0 and pg.SinePE(440).frequency == 440


# ---------------------------------------------------------------------------------------------- the ABI
def test_struct_mirrors_match_c_layout():
    """The sizes pgx_tuning's kernels index by; tests/test_abi.py checks every offset of every struct with a compiler."""
    assert device.TUNING_OP is device._ABI.struct("pgx_tuning_op")
    assert device.TUNING_RECORD is device._ABI.struct("pgx_tuning_record")
    assert device.TUNING_OP.names == ("code", "tuning", "p0", "p1")
    assert device.TUNING_RECORD.names == ("reference_pitch", "reference_freq", "divisions", "table_offset", "num_notes",
                                          "pad")
    assert device.TUNING_OP.itemsize == device.TRANSFORM_OP.itemsize == 24 and device.TUNING_RECORD.itemsize == 40
    assert "pgx_tuning" in device.EXPORTED_SYMBOLS and "pgx_selftest_tuning" in device.EXPORTED_SYMBOLS
