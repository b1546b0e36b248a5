"""
Fixtures for the temperaments and the tuning steps of TransformPE: run the reference's temperament classes and
conversions on the inputs below, render the graph cases through the reference implementation (a started NullRenderer
graph, the caller's blocks) and write tests/golden/tuning_cases.json + tests/golden/tuning.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_tuning.py
The npz holds data only: per "functions" record the float64 result ("fn/<index>"), per graph case the float32 samples of
its blocks ("<name>").  The json holds the inputs, the records (temperament spec, function, reference, input name), what
the reference returns for a scalar and for a list (shape, dtype), every name() / repr(), its validation errors, what each
set_* helper leaves in get_reference_frequency(), and the graph cases with their blocks, their "tuning" verbs (the
globals change before block i) and how each is compared: "bits"; "ulp" -- every sample within one float32 ulp of the
fixture (a float64 result a few ulps off moves the float32 rounding by one step at most); "fuzz" -- audio, where an
oscillator is driven by the stream: per block REL_TOL * peak + ABS_FLOOR (tests/fixture_harness.py).

Checked while generating, against the reference alone:
  * the numpy restatement (pygmu2_amd.temperament through pygmu2_amd.conversions, host code) reproduces every
    "functions" record within 1 ulp (freq_to_pitch: of 128, the size of the sum), with the reference's shapes and dtypes;
  * for every just freq_to_pitch / ratio_to_semitones input -- the records' and the streams' -- no sample has
    log2(ratio) within 1e-9 of an integer, and none has its two smallest |ratios - r| within 1e-9 of each other
    (tuning_oracle.EDGE_CLEARANCE): these outputs are integers plus a constant, there is no "close" for them, so the
    inputs keep clear of the decision edges and the streams are compared to the bit.  An input that violates it is
    replaced (another seed), the clearance stays;
  * just pitch_to_freq streams need no clearance: their floors act on values the device computes with the same IEEE
    operations.
"""

from __future__ import annotations

import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import write_fixture                       # noqa: E402
import tuning_oracle as T                                         # noqa: E402

SR = 44100

ET12 = {"kind": "equal", "divisions": 12}
ET19 = {"kind": "equal", "divisions": 19}
ET53 = {"kind": "equal", "divisions": 53}
JI = {"kind": "just", "ratios": None, "reference_pitch": 60.0}
PYTH = {"kind": "pythagorean", "reference_pitch": 60.0}
JI2 = {"kind": "just", "ratios": [1.0, 1.5], "reference_pitch": 57.0}
JI5 = {"kind": "just", "ratios": [1.0, 9 / 8, 5 / 4, 3 / 2, 5 / 3], "reference_pitch": 57.0}
JI7 = {"kind": "just", "ratios": [1.0, 9 / 8, 5 / 4, 4 / 3, 3 / 2, 5 / 3, 15 / 8], "reference_pitch": 57.0}
TEMPERAMENTS = {"et12": ET12, "et19": ET19, "et53": ET53, "ji": JI, "pyth": PYTH, "ji2": JI2, "ji5": JI5, "ji7": JI7}
REFERENCES = [[f, p] for p in (69.0, 60.0) for f in (440.0, 432.0, 415.0)]


def contig(start, sizes):
    out, s = [], start
    for n in sizes:
        out.append([s, n])
        s += n
    return out


def inputs():
    rng = np.random.default_rng(20)
    boundary = []
    for p in (57.0, 60.0):                                        # either side of an octave boundary of every table
        for n in (2, 5, 7, 12):
            for k in (-1, 0, 1):
                boundary += [p + k * n - 1e-9, p + k * n + 1e-9]
        boundary += [float(np.nextafter(p, -np.inf)), float(np.nextafter(p, np.inf)), p - 1e-15, p - 1e-13]
    pitches = np.concatenate([np.arange(128.0), np.round(rng.uniform(0.0, 127.0, 48), 3), [60.5, 61.25, 71.999],
                              [-0.25, -1.0, -12.0, -23.5, -36.0, -60.0, -0.001], boundary])
    few = np.concatenate([np.arange(0.0, 128.0, 7.0), [60.5, 68.999, -0.25, -13.0], boundary[:12]])
    freqs = np.exp(rng.uniform(np.log(20.0), np.log(12000.0), 96))
    few_freqs = freqs[::6]
    ratios = np.exp(rng.uniform(np.log(0.1), np.log(8.0), 64))
    intervals = np.concatenate([np.arange(-24.0, 49.0), np.round(rng.uniform(-24.0, 48.0, 32), 3), boundary[:12]])
    return {"pitches": pitches, "pitches_few": few, "freqs": freqs, "freqs_few": few_freqs, "ratios": ratios,
            "intervals": intervals}


def function_records():
    recs = []
    for name, spec in TEMPERAMENTS.items():
        for i, ref in enumerate(REFERENCES):
            recs.append({"temperament_name": name, "temperament": spec, "fn": "pitch_to_freq", "reference": ref,
                         "input": "pitches" if i == 0 else "pitches_few"})
            recs.append({"temperament_name": name, "temperament": spec, "fn": "freq_to_pitch", "reference": ref,
                         "input": "freqs" if i == 0 else "freqs_few"})
        recs.append({"temperament_name": name, "temperament": spec, "fn": "semitones_to_ratio", "input": "intervals"})
        recs.append({"temperament_name": name, "temperament": spec, "fn": "ratio_to_semitones", "input": "ratios"})
    return recs


# ---------------------------------------------------------------------------------------------- graph cases
def E(enum, name):
    return {"enum": enum, "name": name}


def piecewise(transition, scale=1.0):
    """Example 33's C major triad, 8 s shrunk to 4096 * scale frames."""
    pts = [[0, 60], [768, 60], [1024, 64], [1792, 64], [2048, 67], [2816, 67], [3072, 60], [3840, 60]]
    pts = [[int(round(t * scale)), p] for t, p in pts]
    return {"type": "PiecewisePE", "args": [pts],
            "kwargs": {"transition_type": E("TransitionType", transition), "extend_mode": E("ExtendMode", "HOLD_LAST")}}


def transform(source, func=None, partial=None, ops=None):
    node = {"type": "Transform", "source": source}
    if ops is not None:
        node["ops"] = ops
    else:
        node["func"] = func
        if partial is not None:
            node["partial"] = partial
    return node


def array(seed, lo, hi, ch=1, n=1500):
    return {"type": "Array", "seed": seed, "n": n, "ch": ch, "lo": lo, "hi": hi}


def node(kind, *args, **kwargs):
    return {"type": kind, "args": list(args), "kwargs": kwargs}


LONG = contig(0, [1, 63, 64, 65, 257, 1000, 1000, 1646])           # 4096 frames
SHORT = contig(0, [1, 63, 64, 65, 257, 1000])                      # 1450 frames


def cases():
    c = []

    def add(name, graph, blocks, compare, **extra):
        c.append(dict({"name": name, "sr": SR, "graph": graph, "blocks": blocks, "compare": compare}, **extra))

    # example 33: piecewise pitch -> pitch_to_freq (the function itself) -> sawtooth, the stream alone and the audio
    for transition in ("STEP", "LINEAR"):
        freq = transform(piecewise(transition), "pitch_to_freq")
        add(f"ex33_{transition.lower()}_freq", freq, LONG, "ulp")
        saw = node("FunctionGenPE", frequency=freq, duty_cycle=0.5, waveform="sawtooth")
        add(f"ex33_{transition.lower()}_audio", node("GainPE", saw, 0.25), LONG, "fuzz")
    # the same glide under other temperaments, A4 = 432: keyword-only partials of the function
    for name in ("ji", "pyth", "et19", "ji5"):
        add(f"glide_{name}_432", transform(piecewise("LINEAR", 1450 / 4096), "pitch_to_freq",
                                           {"temperament": TEMPERAMENTS[name], "reference_freq": 432.0}), SHORT, "ulp")
    # 2 and 3 channels, every table size, negative and fractional pitches
    for ch, name in ((2, "ji"), (3, "ji7"), (2, "ji2"), (3, "et53")):
        add(f"array_{ch}ch_{name}", transform(array(30 + ch, -30.0, 130.0, ch), ops=[
            ["pitch_to_freq", TEMPERAMENTS[name], 69.0, 440.0]]), SHORT, "ulp")
    add("chain_affine_pitch_clip", transform(array(41, -1.0, 1.0), ops=[
        ["affine", 12.0, 60.0], ["pitch_to_freq", PYTH, 69.0, 440.0], ["clip", 200.0, 400.0]]), SHORT, "ulp")
    # semitones_to_ratio: a +-0.5 semitone vibrato as a gain; the ratio streams themselves
    vib = transform(node("SinePE", 5.0), ops=[["affine", 0.5, 0.0], ["semitones_to_ratio", None]])
    add("vibrato_gain", node("GainPE", node("SinePE", 440.0), vib), SHORT, "fuzz")
    add("ratio_et12", transform(array(42, -24.0, 24.0), "semitones_to_ratio"), SHORT, "ulp")
    add("ratio_ji", transform(array(43, -24.0, 24.0, 2), "semitones_to_ratio", {"temperament": JI}), SHORT, "ulp")
    # the inverse streams: equal (a logarithm: one ulp), just (a table index: to the bit; one channel -- the reference's
    # nearest-entry loop walks the rows of its input and only takes rows of one sample)
    add("pitch_et12", transform(array(44, 50.0, 4000.0), "freq_to_pitch"), SHORT, "ulp")
    add("pitch_et19_432", transform(array(45, 50.0, 4000.0, 2), "freq_to_pitch",
                                    {"temperament": ET19, "reference_freq": 432.0}), SHORT, "ulp")
    add("pitch_ji", transform(array(46, 50.0, 4000.0), "freq_to_pitch", {"temperament": JI}), SHORT, "bits",
        just={"temperament": JI, "reference": [440.0, 69.0]})
    add("pitch_ji5_415", transform(array(47, 50.0, 4000.0), ops=[["freq_to_pitch", JI5, 60.0, 415.0]]), SHORT, "bits",
        just={"temperament": JI5, "reference": [415.0, 60.0]})
    add("semitones_et12", transform(array(48, 0.25, 4.0), "ratio_to_semitones"), SHORT, "ulp")
    add("semitones_ji7", transform(array(49, 0.25, 4.0), "ratio_to_semitones", {"temperament": JI7}), SHORT, "bits",
        just={"temperament": JI7, "reference": None})
    # the globals change before the third block: the function follows them from that block on
    add("global_change", transform(piecewise("LINEAR", 1450 / 4096), "pitch_to_freq"),
        contig(0, [64, 64, 65, 257, 1000]), "ulp",
        ops={"2": {"tuning": {"temperament": JI, "reference": [432.0, 69.0]}}})
    # example 20's C major chord in its three temperaments
    for name in ("et12", "ji", "pyth"):
        sines = [node("SinePE", frequency={"type": "Freq", "pitch": n, "keywords": {"temperament": TEMPERAMENTS[name]}},
                      amplitude=0.2 / 3) for n in (60, 64, 67)]
        add(f"ex20_chord_{name}", node("CropPE", node("MixPE", *sines), 0, 2048),
            contig(0, [1, 63, 64, 65, 257, 1000, 598]), "fuzz")
    return c


# ---------------------------------------------------------------------------------------------- the reference
def reference_namespace(mods):
    M = mods["K"]
    tm = importlib.import_module("pygmu2.temperament")
    for name, value in vars(tm).items():
        if not name.startswith("_") and getattr(value, "__module__", None) == tm.__name__:
            setattr(M, name, value)
    for name in T.FUNCTIONS:
        setattr(M, name, getattr(mods["conversions"], name))
    M.transform = lambda ops: T.numpy_chain(M, ops)
    return M


def facts(M):
    """Shapes and dtypes for a scalar and a list, names, reprs, validation errors, the set_* helpers."""
    out = {"temperaments": {}, "errors": {}, "helpers": {}}
    for name, spec in TEMPERAMENTS.items():
        t = T.temperament(M, spec)
        shapes = {}
        for fn, scalar in (("pitch_to_freq", 60), ("freq_to_pitch", 300.0), ("interval_to_ratio", 7),
                           ("ratio_to_interval", 1.4)):
            shapes[fn] = {"scalar": T.shape_of(getattr(t, fn), scalar),
                          "list": T.shape_of(getattr(t, fn), [scalar, scalar * 1.01])}
        out["temperaments"][name] = {"name": t.name(), "repr": repr(t), "shapes": shapes,
                                     "num_notes": getattr(t, "num_notes", None), "divisions": getattr(t, "divisions", None)}
    custom = M.CustomTemperament(None, None, None, None, name="Stretched")
    out["temperaments"]["custom"] = {"name": custom.name(), "repr": repr(custom)}
    out["temperaments"]["custom_default"] = {"name": M.CustomTemperament(None, None, None, None).name()}
    refusals = {"divisions_zero": lambda: M.EqualTemperament(0),
                "one_ratio": lambda: M.JustIntonation([1.0]),
                "no_unison": lambda: M.JustIntonation([1.1, 1.5]),
                "reference_zero": lambda: M.set_reference_frequency(0.0),
                "reference_negative": lambda: M.set_reference_frequency(-440.0, 60.0)}
    for key, make in refusals.items():
        try:
            make()
            raise AssertionError(f"{key}: the reference accepts it")
        except ValueError as e:
            out["errors"][key] = {"type": type(e).__name__, "text": str(e)}
    out["helpers"]["initial"] = list(M.get_reference_frequency())
    out["initial_temperament"] = repr(M.get_temperament())
    for helper in ("set_verdi_tuning", "set_baroque_pitch", "set_concert_pitch"):
        getattr(M, helper)()
        out["helpers"][helper] = list(M.get_reference_frequency())
    M.set_reference_frequency(442, 57)
    out["helpers"]["set_reference_frequency(442, 57)"] = [repr(v) for v in M.get_reference_frequency()]
    M.set_concert_pitch()
    return out


def restatement():
    import pygmu2_amd as pg
    pg.set_sample_rate(SR)
    return T.package_namespace()


def check_just_clearance(P, where, spec, reference, values):
    t = T.temperament(P, spec)
    base = 1.0 if reference is None else float(t._base_freq(reference[1], reference[0])[0])
    log_gap, tie_gap = T.just_clearance(t.ratios, np.maximum(np.asarray(values, np.float64), 1e-10) / base)
    assert log_gap > T.EDGE_CLEARANCE and tie_gap > T.EDGE_CLEARANCE, \
        f"{where}: an input lies {log_gap:g} from an octave edge / {tie_gap:g} from a tie: choose another input"
    return log_gap, tie_gap


def main():
    mods = gen_golden.load_reference()
    mods["config"].set_sample_rate(SR)
    M = reference_namespace(mods)
    P = restatement()
    arrays, ins = {}, inputs()
    doc = {"inputs": {k: [float(x) for x in v] for k, v in ins.items()}, "functions": function_records()}
    doc.update(facts(M))
    worst = 0.0
    for i, rec in enumerate(doc["functions"]):
        values = doc["inputs"][rec["input"]]
        want = np.asarray(T.call_function(M, rec, values))
        got = np.asarray(T.call_function(P, rec, values))
        assert want.dtype == np.float64 and got.dtype == np.float64 and want.shape == got.shape, rec
        scale = np.spacing(128.0) if rec["fn"] == "freq_to_pitch" else np.spacing(np.abs(want))
        if rec["fn"] == "ratio_to_semitones":
            scale = np.spacing(np.maximum(np.abs(want), 1.0))
        err = float(np.max(np.abs(got - want) / scale))
        worst = max(worst, err)
        assert err <= 1.0, f"{rec}: the restatement is {err} ulp from the reference"
        if rec["temperament"]["kind"] != "equal" and rec["fn"] in ("freq_to_pitch", "ratio_to_semitones"):
            check_just_clearance(P, f"functions[{i}]", rec["temperament"], rec.get("reference"), values)
        arrays[f"fn/{i}"] = want
    print(f"{len(doc['functions'])} function records, the restatement at most {worst} ulp away")
    all_cases = cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs = T.render_case(M, case, mods["null_renderer"].NullRenderer(sample_rate=case["sr"]))
        flat = np.concatenate(outs)
        assert flat.dtype == np.float32 and np.all(np.isfinite(flat)), case["name"]
        if "just" in case:
            src = T.array_data(case["graph"]["source"]).astype(np.float64)
            gaps = check_just_clearance(P, case["name"], case["just"]["temperament"], case["just"]["reference"], src)
            print(f"{case['name']}: clear of the edges by {gaps[0]:.3g} (octave) / {gaps[1]:.3g} (tie)")
        else:
            assert case["compare"] != "bits", case["name"]
        arrays[case["name"]] = flat
        print(f"{case['name']}: {flat.shape} {case['compare']} peak {float(np.max(np.abs(flat))):.6g}", flush=True)
    doc["cases"] = all_cases
    write_fixture("tuning", doc, arrays)


if __name__ == "__main__":
    main()
