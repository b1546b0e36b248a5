"""GPU: the tuning steps of TransformPE (pgx_tuning) against fixtures of the reference (tests/golden/tuning_cases.json,
tuning.npz), the device functions in float64 against numpy on this machine (pgx_selftest_tuning), and what the lowered
path promises: no host copy of a block, the old launch for chains without a tuning step, and the new tuning in the first
block rendered after the globals changed."""

import numpy as np
import pytest

import pygmu2_amd as pg
from pygmu2_amd import device, read_ahead, transform_pe, transforms
from pygmu2_amd.snippet import Snippet
import fixture_harness as H
import tuning_oracle as T

pytestmark = pytest.mark.gpu

DATA, NPZ = H.load_cases("tuning")
CASES = DATA["cases"]
M = T.package_namespace()
TEMPERAMENTS = {r["temperament_name"]: r["temperament"] for r in DATA["functions"]}


@pytest.fixture(autouse=True)
def _default_tuning():
    T.default_tuning(pg)
    yield
    T.default_tuning(pg)


def assert_one_ulp(name, got, want):
    """Every sample within one float32 ulp of the fixture: a float64 result a few float64 ulps off can only move the
    float32 rounding by one step, and only when it sits within 2^-27 of a rounding boundary."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    differ = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    print(f"ULP {name} differing={differ} of {got.size} worst={float(np.max(err / ulp)):.3g} ulp")
    assert np.all(err <= ulp), f"{name}: {int(np.sum(err > ulp))} samples more than one float32 ulp away"


def check_case(case):
    outs = T.render_case(M, case, pg.NullRenderer(sample_rate=case["sr"]))
    stored = H.split_blocks(case, NPZ[case["name"]])
    assert len(stored) == len(outs)
    if case["compare"] == "bits":
        for i, want in stored.items():
            H.assert_bits(f"{case['name']} block {i}", outs[i], want)
    elif case["compare"] == "ulp":
        for i, want in stored.items():
            assert_one_ulp(f"{case['name']} block {i}", outs[i], want)
    else:
        assert case["compare"] == "fuzz", case["compare"]
        H.assert_per_block(case["name"], outs, stored, H.REL_TOL, H.ABS_FLOOR, "TUNING")
    return outs


@pytest.mark.parametrize("case", [c for c in CASES if "ops" not in c], ids=lambda c: c["name"])
def test_graph_cases_match_the_reference(case):
    check_case(case)


@pytest.mark.parametrize("ahead", [True, False], ids=["read_ahead", "no_read_ahead"])
def test_the_block_after_a_tuning_change_carries_the_new_tuning(ahead):
    case = next(c for c in CASES if c["name"] == "global_change")
    change = int(next(iter(case["ops"])))
    was = read_ahead.enabled()
    read_ahead.set_enabled(ahead)
    try:
        outs = check_case(case)
    finally:
        read_ahead.set_enabled(was)
    # the fixture's own samples say that the change is audible in that very block
    start, n = case["blocks"][change]
    pitch = T.build_graph(M, case["graph"]["source"]).render(start, n).data.astype(np.float64)
    old = pg.pitch_to_freq(pitch).astype(np.float32)
    assert np.all(np.abs(outs[change] - old) > 1.0)


def _recording_lib(monkeypatch):
    """transform_pe's library handle replaced by one that notes which entry points are called."""
    real, calls = transform_pe.lib(), []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(transform_pe, "lib", lambda: Recorder())
    return calls


def test_a_lowered_pitch_to_freq_makes_no_host_copy(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a lowered tuning step touched the host")
    pitch = pg.PiecewisePE([(0, 60.0), (500, 72.0)], extend_mode=pg.ExtendMode.HOLD_LAST)
    pe = pg.TransformPE(pitch, func=pg.pitch_to_freq)
    saw = pg.FunctionGenPE(frequency=pe, waveform="sawtooth")
    calls = _recording_lib(monkeypatch)
    monkeypatch.setattr(pg.TransformPE, "_render_host_callable", refuse)
    monkeypatch.setattr(Snippet, "data", property(refuse))
    monkeypatch.setattr(device.DeviceBuffer, "to_host", refuse)
    snips = [saw.render(i * 257, 257) for i in range(3)] + [pe.render(0, 600)]
    monkeypatch.undo()
    assert calls and set(calls) == {"pgx_tuning"}
    got = snips[-1].data
    want = pg.pitch_to_freq(pitch.render(0, 600).data.astype(np.float64)).astype(np.float32)
    assert_one_ulp("lowered pitch_to_freq", got, want)


def test_a_chain_without_a_tuning_step_still_launches_pgx_transform(monkeypatch):
    src = pg.ArrayPE(T.array_data({"seed": 5, "n": 300, "ch": 2, "lo": -2.0, "hi": 2.0}))
    chain = transforms.Chain(transforms.Affine(0.5, 0.25), transforms.Tanh(), transforms.Square())
    calls = _recording_lib(monkeypatch)
    plain = pg.TransformPE(src, func=chain).render(0, 300).data
    assert set(calls) == {"pgx_transform"}
    del calls[:]
    tuned = pg.TransformPE(src, func=transforms.Chain(*chain.steps, transforms.SemitonesToRatio(pg.EqualTemperament(12))))
    tuned.render(0, 300)
    assert set(calls) == {"pgx_tuning"}
    want = np.tanh(0.25 + 0.5 * src.render(0, 300).data.astype(np.float64)) ** 2
    assert np.max(np.abs(plain - want.astype(np.float32))) <= np.spacing(np.float32(1.0))


def test_codes_0_to_6_give_pgx_transform_s_bytes():
    """One launch of each kernel over the same op table, no tuning op in it: the two switch bodies are the same code."""
    lib = device.ensure_init()
    x = T.array_data({"seed": 6, "n": 1000, "ch": 1, "lo": -3.0, "hi": 3.0}).reshape(-1)
    ops = np.zeros(7, dtype=device.TRANSFORM_OP)
    for i, (code, p0, p1) in enumerate([(0, 0.7, 0.1), (4, 0, 0), (2, 0, 0), (5, 0, 0), (3, 0, 0), (6, 0, 0),
                                        (1, 0.2, 0.9)]):
        ops[i] = (code, 0, p0, p1)
    xd, od = device.DeviceBuffer.from_host(x), device.DeviceBuffer.from_host(ops.view(np.uint8))
    a, b = device.DeviceBuffer(x.shape, np.float32), device.DeviceBuffer(x.shape, np.float32)
    records = device.DeviceBuffer.from_host(np.zeros(1, dtype=device.TUNING_RECORD).view(np.uint8))
    tables = device.DeviceBuffer.from_host(np.zeros(1))
    device.check(lib.pgx_transform(a.ptr, xd.ptr, x.size, od.ptr, 7), "pgx_transform")
    device.check(lib.pgx_tuning(b.ptr, xd.ptr, x.size, od.ptr, 7, records.ptr, tables.ptr), "pgx_tuning")
    H.assert_bits("codes 0-6", b.to_host(), a.to_host())


# ---------------------------------------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("notes", [2, 5, 12, 53])
def test_small_shapes_and_table_sizes(notes):
    """n_elems in {1, 63, 64, 65, 257} x channels {1, 2, 3}: where an index, a wrap or a tail can go wrong.  Tables of
    N entries: an equal-tempered scale written as a ratio table, so the expected stream needs no reference."""
    ratios = 2.0 ** (np.arange(notes) / notes)
    ratios[0] = 1.0
    ji = pg.JustIntonation(ratios, reference_pitch=57.0)
    forward = transforms.PitchToFreq(ji, 69.0, 440.0)
    for ch in (1, 2, 3):
        for n in (1, 63, 64, 65, 257):
            data = T.array_data({"seed": 100 * ch + n, "n": n, "ch": ch, "lo": -40.0, "hi": 140.0})
            data[0, 0] = 57.0 + notes                            # exactly on the octave
            got = pg.TransformPE(pg.ArrayPE(data), func=forward).render(0, n).data
            want = forward(data.astype(np.float64)).astype(np.float32)
            assert_one_ulp(f"N={notes} ch={ch} n={n}", got, want)
            # a frame beyond the source's extent is pitch 0
            tail = pg.TransformPE(pg.ArrayPE(data), func=forward).render(n - 1, 3).data
            assert tail.shape == (3, ch) and np.all(tail[1:] == np.float32(forward(np.zeros(1))[0]))


# ---------------------------------------------------------------------------------------------- float64 accuracy
def _selftest(code, tuning, x):
    lib = device.ensure_init()
    rec = np.zeros(1, dtype=device.TUNING_RECORD)
    notes = 0 if not tuning.just else (len(tuning.table) - 1) // 2
    rec[0] = (tuning.reference_pitch, tuning.reference_freq, tuning.divisions, 0, notes, 0)
    records = device.DeviceBuffer.from_host(rec.view(np.uint8))
    tables = device.DeviceBuffer.from_host(np.asarray(tuning.table if tuning.just else np.zeros(1), dtype=np.float64))
    xd, out = device.DeviceBuffer.from_host(x), device.DeviceBuffer(x.shape, np.float64)
    device.check(lib.pgx_selftest_tuning(out.ptr, xd.ptr, x.size, code, records.ptr, tables.ptr), "pgx_selftest_tuning")
    return out.to_host()


def _just_inverse(t, inverse, x):
    """JustIntonation's nearest-entry loop over all rows at once (np.argmin along an axis takes the first minimum too)."""
    base = 1.0 if inverse.reference_pitch is None else float(t._base_freq(inverse.reference_pitch, inverse.reference_freq)[0])
    ratio = np.maximum(x, 1e-10) / base
    octaves = np.floor(np.log2(ratio))
    degrees = np.argmin(np.abs(t.ratios[None, :] - (ratio / 2.0 ** octaves)[:, None]), axis=1)
    own = 0.0 if inverse.reference_pitch is None else t._reference_pitch
    return own + (octaves * t.num_notes + degrees)


@pytest.fixture(scope="module")
def selftest_inputs():
    rng = np.random.default_rng(23)
    ins = {k: np.asarray(v, dtype=np.float64) for k, v in DATA["inputs"].items()}
    return {"pitches": np.concatenate([ins["pitches"], ins["intervals"], rng.uniform(-24.0, 152.0, 100_000)]),
            "freqs": np.concatenate([ins["freqs"], rng.uniform(8.0, 20000.0, 100_000)]),
            "ratios": np.concatenate([ins["ratios"], rng.uniform(8.0, 20000.0, 100_000) / 440.0])}


@pytest.mark.parametrize("name", sorted(TEMPERAMENTS))
def test_device_functions_against_numpy(name, selftest_inputs):
    """The exp2 paths <= 4 ulp, the log2 paths <= 4 * spacing(128) absolute: the bound tests/test_gpu_math.py holds the
    library's sin/cos and tanh to.  The measured maxima are printed (DESIGN.md quotes them)."""
    t = T.temperament(pg, TEMPERAMENTS[name])
    bound = 4 * np.spacing(128.0)
    for ref in ((69.0, 440.0), (60.0, 415.0), None):
        forward = transforms.PitchToFreq(t, *ref) if ref else transforms.SemitonesToRatio(t)
        inverse = transforms.FreqToPitch(t, *ref) if ref else transforms.RatioToSemitones(t)
        (code, tuning, _), = forward.ops()
        x = selftest_inputs["pitches"]
        got, want = _selftest(code, tuning, x), np.asarray(forward(x)).reshape(-1)
        ulps = float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))
        print(f"SELFTEST {name} ref={ref} exp2 path: {ulps:.3g} ulp")
        assert ulps <= 4.0
        (code, tuning, _), = inverse.ops()
        x = selftest_inputs["freqs" if ref else "ratios"]
        if tuning.just:
            want = _just_inverse(t, inverse, x)
            assert np.array_equal(want[:64], np.asarray(inverse(x[:64].reshape(-1, 1))).reshape(-1))
        else:
            want = np.asarray(inverse(x)).reshape(-1)
        got = _selftest(code, tuning, x)
        err = float(np.max(np.abs(got - want)))
        print(f"SELFTEST {name} ref={ref} log2 path: {err:.3g} absolute = {err / np.spacing(128.0):.3g} spacing(128)")
        assert err <= bound


def test_selftest_edge_values():
    ji = pg.JustIntonation(reference_pitch=0.0)
    (code, tuning, _), = transforms.SemitonesToRatio(ji).ops()
    x = np.array([-5e-16, 0.0, 12.0, 11.999999999999998, -12.0, np.nan, np.inf, -np.inf, 1e300, 23.5])
    got = _selftest(code, tuning, x)
    with np.errstate(all="ignore"):
        want = ji.interval_to_ratio(x[[0, 1, 2, 3, 4, 9]])
    assert got[0] == 0.5 and got[1] == 1.0                       # the scale degree that rounds to N: the lower octave
    assert np.max(np.abs(got[[0, 1, 2, 3, 4, 9]] - want) / np.spacing(want)) <= 4.0
    assert np.all(np.isnan(got[5:8]))                            # no table index for these: NaN, nothing read
    assert got[8] == np.inf                                      # degree 0 of an octave beyond the range, as numpy
    (code, tuning, _), = transforms.RatioToSemitones(ji).ops()
    got = _selftest(code, tuning, np.array([0.0, -3.0, 1e-10, 1.0, 2.0, 0.5, np.nan]))
    floor = ji.ratio_to_interval(np.array([1e-10]))[0]
    assert got[:6].tolist() == [floor, floor, floor, 0.0, 12.0, -12.0] and np.isnan(got[6])
