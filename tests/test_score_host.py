"""CPU: SequencePE's construction facts and error texts and the unit conversions against what the reference recorded
(tests/golden/score_cases.json), the score bank's note classifier on hand-made graphs, and its host tables (the cull,
the per-tile lists) against brute force on random scores.  Nothing here touches the device."""

import types

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import score_bank
from fixture_harness import load_cases
from score_oracle import SR, brute_active, brute_tile_lists, build_case
from spec_build import PG

DATA, _ = load_cases("score")
CASES = DATA["cases"]


@pytest.fixture(autouse=True)
def _rate():
    pg.set_sample_rate(SR)


# ---------------------------------------------------------------------------------------------- SequencePE
@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "sequence"], ids=lambda c: c["name"])
def test_sequence_facts_match_the_reference(case):
    pe = build_case(PG, case)
    want = case["pe"]
    ext = pe.extent()
    assert repr(pe) == want["repr"]
    assert [ext.start, ext.end] == want["extent"]
    assert pe.is_pure() == want["pure"]
    assert pe.channel_count() == want["channels"]
    assert [type(i).__name__ for i in pe.inputs()] == want["inputs"]
    assert [type(i).__name__ for i in pe.inputs()[0].inputs()] == want["inner_inputs"]
    assert pe.mode.value == want["mode"] and isinstance(pe.mode, pg.SequenceMode)
    assert [[type(p).__name__, int(s)] for p, s in pe._pairs] == want["pairs"]


def _refusals():
    mk = lambda: pg.CropPE(pg.SinePE(100.0), 0, 10)                 # noqa: E731
    return {
        "no_pairs": lambda: pg.SequencePE(),
        "empty_list": lambda: pg.SequencePE([]),
        "not_a_pair": lambda: pg.SequencePE((mk(), 0), mk()),
        "triple": lambda: pg.SequencePE((mk(), 0, 1), (mk(), 2)),
        "auto_after_infinite": lambda: pg.SequencePE((pg.SinePE(100.0), 0), (mk(), None)),
        "bad_mode": lambda: pg.SequencePE((mk(), 0), (mk(), 5), mode="legato"),
    }


@pytest.mark.parametrize("name", sorted(DATA["refused"]))
def test_refused_constructions_raise_the_reference_error(name):
    want = DATA["refused"][name]
    with pytest.raises(Exception) as info:
        _refusals()[name]()
    assert type(info.value).__name__ == want["type"]
    assert str(info.value) == want["text"]


def test_pluck_sequence_is_pure_like_the_reference():
    seq = pg.SequencePE((pg.CropPE(pg.KarplusStrongPE(220.0, seed=1), 0, 100), 0),
                        (pg.CropPE(pg.KarplusStrongPE(330.0, seed=2), 0, 100), None))
    assert seq.is_pure() is True and not seq.inputs()[0].inputs()[0].inputs()[0].inputs()[0].is_pure()
    assert [s for _, s in seq._pairs] == [0, 100]


def test_equal_starts_give_a_zero_length_crop():
    a, b, c = (pg.CropPE(pg.SinePE(100.0 * k), 0, 50) for k in (1, 2, 3))
    seq = pg.SequencePE((a, 10), (b, 10), (c, 40), mode="Non_Overlap")
    first = seq.inputs()[0].inputs()[0]
    assert isinstance(first, pg.CropPE) and first.duration == 0 and first.extent().is_empty()
    assert seq.mode is pg.SequenceMode.NON_OVERLAP


# ---------------------------------------------------------------------------------------------- conversions
def _ulps(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.max(np.abs(got - want) / np.spacing(np.abs(want)))


def test_conversions_match_the_reference():
    c = DATA["conversions"]
    # 2.0 ** and log2 go through libm, whose last bit may differ between builds: within 1 ulp
    assert _ulps(pg.pitch_to_freq(c["midi"]), c["pitch_to_freq"]) <= 1
    assert _ulps(pg.semitones_to_ratio(c["semitones"]), c["semitones_to_ratio"]) <= 1
    got = pg.freq_to_pitch(c["pitch_to_freq"])
    assert np.max(np.abs(got - np.asarray(c["freq_to_pitch"])) / np.spacing(128.0)) <= 1      # an ulp of the sum's size
    got = pg.ratio_to_semitones(c["ratios"])
    want = np.asarray(c["ratio_to_semitones"])
    assert np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(want), 1.0)))
    # one multiplication / division: exact
    for rate, want_n, want_s in zip(c["rates"], c["seconds_to_samples"], c["samples_to_seconds"]):
        assert pg.seconds_to_samples(c["seconds"], rate).tolist() == want_n
        assert pg.samples_to_seconds(c["samples"], rate).tolist() == want_s
    assert type(pg.pitch_to_freq(69)).__name__ == c["scalar_type"]
    assert str(pg.pitch_to_freq([69]).dtype) == c["array_dtype"] == "float64"
    assert pg.pitch_to_freq(69) == 440.0 and pg.freq_to_pitch(440.0) == 69.0
    assert pg.semitones_to_ratio(12) == 2.0 and pg.ratio_to_semitones(0.5) == -12.0


@pytest.mark.parametrize("fn", ["pitch_to_freq", "freq_to_pitch", "semitones_to_ratio", "ratio_to_semitones"])
def test_conversions_refuse_a_temperament(fn):
    with pytest.raises(NotImplementedError, match="temperament"):
        getattr(pg, fn)(60.0, temperament=object())


def test_new_names_are_bound_and_not_exported():
    names = ["SequencePE", "SequenceMode", "pitch_to_freq", "freq_to_pitch", "semitones_to_ratio",
             "ratio_to_semitones", "samples_to_seconds", "seconds_to_samples", "score_bank"]
    for name in names:
        assert hasattr(pg, name), name
        assert name not in pg.__all__, name
    assert pg.ratio_to_db is pg.dynamics_pe.ratio_to_db and pg.db_to_ratio is pg.dynamics_pe.db_to_ratio


# ---------------------------------------------------------------------------------------------- the classifier
def _ks(seed=1):
    return pg.KarplusStrongPE(220.0, seed=seed)


def test_classifier_accepts_each_layer_kind():
    core = _ks()
    got = score_bank.classify(pg.DelayPE(pg.CropPE(core, 0, 300), 1000))
    assert got[0] is core and got[1:4] == (1000, 1000, 1300) and len(got[4]) == 2
    core = _ks()
    got = score_bank.classify(pg.CropPE(pg.DelayPE(core, 500), 500, 200))             # NON_OVERLAP's shape
    assert got[0] is core and got[1:4] == (500, 500, 700)
    core = pg.SinePE(100.0)
    nested = pg.DelayPE(pg.CropPE(pg.DelayPE(pg.CropPE(core, -50, 400), -20), 0, 100), 7)
    got = score_bank.classify(nested)                # [-50, 350) - 20 -> [-70, 330), cut to [0, 100), + 7
    assert got[0] is core and got[1:4] == (-13, 7, 107)
    arr = pg.ArrayPE(np.zeros((100, 2), dtype=np.float32))
    assert score_bank.classify(pg.CropPE(arr, 10, 50))[1:4] == (0, 10, 60)
    assert score_bank.classify(pg.DelayPE(pg.CropPE(arr, 10, 50), 2.0))[1:4] == (2, 12, 62)     # 2.0 is an integer delay
    empty = score_bank.classify(pg.CropPE(pg.CropPE(_ks(), 0, 10), 20, 10))
    assert empty[2] == empty[3]                       # crops that miss each other: a note that never sounds


def test_classifier_rejects_each_disqualifier():
    arr = pg.ArrayPE(np.zeros((100, 1), dtype=np.float32))
    assert score_bank.classify(_ks()) is None                                          # no window at all
    assert score_bank.classify(pg.DelayPE(arr, 10)) is None                            # bounded core, no crop
    assert score_bank.classify(pg.DelayPE(_ks(), 100)) is None                         # the unbounded tail element
    assert score_bank.classify(pg.CropPE(_ks(), 0, None)) is None                      # open end
    assert score_bank.classify(pg.CropPE(_ks(), -10, 100)) is None                     # window leaves the core's extent
    assert score_bank.classify(pg.CropPE(arr, 50, 100)) is None
    assert score_bank.classify(pg.DelayPE(pg.CropPE(_ks(), 0, 100), 2.5)) is None      # fractional delay
    assert score_bank.classify(pg.DelayPE(pg.CropPE(_ks(), 0, 100), pg.ConstantPE(3.0))) is None     # PE delay
    assert score_bank.classify(pg.CropPE(_ks(), 0, 100, pg.ExtendMode.HOLD_LAST)) is None
    assert score_bank.classify(pg.GainPE(pg.CropPE(_ks(), 0, 100), 0.5)) is None       # another PE on top
    # a filter whose ring-out leaves its extent: BiquadPE's extent is its source's, the crop around it asks for more
    ringing = pg.BiquadPE(pg.CropPE(pg.SinePE(100.0), 0, 100), frequency=500.0, q=5.0)
    assert score_bank.classify(pg.CropPE(ringing, 0, 300)) is None


def test_bank_needs_two_notes_and_yields_to_the_voice_bank(monkeypatch):
    notes = [pg.DelayPE(pg.CropPE(_ks(i), 0, 100), 50 * i) for i in range(3)]
    assert pg.MixPE(*notes)._score_bank().n_notes == 3
    mix = pg.MixPE(notes[0], pg.SinePE(100.0), pg.DelayPE(_ks(9), 5))
    assert mix._score_bank() is False and mix._score is False
    tail = pg.MixPE(notes[1], notes[2], pg.DelayPE(_ks(9), 5))
    assert tail._score_bank().n_notes == 2 and tail._score_bank()._whole == [2]
    # _read_ahead_condition / _look_ahead_condition answer as before
    assert pg.MixPE(*[pg.DelayPE(pg.CropPE(_ks(i), 0, 100), 50 * i) for i in range(3)])._read_ahead_condition() is False
    # a mix the voice bank takes never asks the score bank
    calls = []
    monkeypatch.setattr(score_bank, "try_build_score", lambda inputs: calls.append(1))
    voiced = pg.MixPE(*[pg.DelayPE(pg.CropPE(_ks(i), 0, 100), 50 * i) for i in range(3)])
    voiced._bank = types.SimpleNamespace(render_mix=lambda s, d: "voice bank")
    assert voiced._render(0, 16) == "voice bank" and not calls
    # switched off: not built
    monkeypatch.undo()
    score_bank.set_enabled(False)
    try:
        off = pg.MixPE(*[pg.DelayPE(pg.CropPE(_ks(i), 0, 100), 50 * i) for i in range(3)])
        assert off._score_bank() is False and off._score is None
    finally:
        score_bank.set_enabled(True)


# ---------------------------------------------------------------------------------------------- host tables
@pytest.mark.parametrize("seed", range(6))
def test_cull_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 400))
    starts = np.sort(rng.integers(-5000, 50_000, k)).astype(np.int64)
    ends = starts + rng.integers(1, 3000 if seed % 2 else 30_000, k)
    run_max = np.maximum.accumulate(ends)
    for _ in range(200):
        a = int(rng.integers(-8000, 60_000))
        b = a + int(rng.integers(1, 5000))
        got = score_bank.cull(starts, ends, run_max, a, b).tolist()
        assert got == brute_active(starts, ends, a, b)


def test_bank_active_is_in_input_order_and_skips_empty_notes():
    starts = [400, 0, 400, 100, 250]
    lens = [100, 150, 0, 500, 10]
    notes = [pg.DelayPE(pg.CropPE(_ks(i), 0, n), s) for i, (s, n) in enumerate(zip(starts, lens))]
    bank = pg.MixPE(*notes)._score_bank()
    assert bank.active(0, 1000).tolist() == [0, 1, 3, 4]
    assert bank.active(140, 20).tolist() == [1, 3]
    assert bank.active(600, 50).tolist() == [] and bank.active(-100, 100).tolist() == []
    assert bank.active(499, 2).tolist() == [0, 3]


@pytest.mark.parametrize("seed", range(5))
def test_tile_lists_match_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    n_frames = int(rng.integers(1, 9000))
    tile = int(rng.choice([1, 7, 256, 1024]))
    k = int(rng.integers(1, 120))
    first = rng.integers(0, n_frames, k)
    frames = np.minimum(rng.integers(1, 2 * tile + 50, k), n_frames - first)
    for edge in range(0, min(k, 12), 3):                  # ends one frame either side of a tile boundary
        t = tile * int(rng.integers(1, n_frames // tile + 1)) if n_frames > tile else n_frames
        first[edge], frames[edge] = 0, max(1, min(n_frames, t - 1))
        if edge + 1 < k:
            first[edge + 1], frames[edge + 1] = 0, max(1, min(n_frames, t + 1))
    offsets, entries = score_bank.tile_lists(first, frames, n_frames, tile)
    want = brute_tile_lists(first.tolist(), frames.tolist(), n_frames, tile)
    assert offsets.dtype == np.int32 and entries.dtype == np.int32 and offsets[0] == 0
    assert len(offsets) == len(want) + 1 and offsets[-1] == len(entries)
    for t, members in enumerate(want):
        assert entries[offsets[t]:offsets[t + 1]].tolist() == members
    assert len(entries) <= int(np.sum(frames // tile + 2))
