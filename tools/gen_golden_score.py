"""
Fixtures for SequencePE, the unit conversions and the score bank: render the cases below through the reference
implementation on the CPU (a started NullRenderer graph, the caller's blocks, a fresh graph per block pattern) and
write tests/golden/score_cases.json + tests/golden/score.npz.

Needs the reference package (oracle.gen_golden.load_reference; sequence_pe and noise_pe are imported next to it).  Run
from the repository root:
    python tools/gen_golden_score.py
The npz holds data only: per case the reference's whole render ("<case>/whole") and every other block pattern whose
output is NOT what the whole render holds over the same frames ("<case>/<pattern>": the patterns that seek backward
over notes that carry state); for the rest the json says so ("same_as_whole") and the tests cut the whole render.  The
json holds the cases (note sources, starts, mode, argument form, block patterns), per SequencePE the reference's
extent / repr / purity / channel count / input type names / sorted (type, start) pairs, the exception type and text of
every refused construction, and the six conversions at MIDI 0..127 and at a handful of ratios and times.

Checked while generating, against the reference alone: a SequencePE of pluck notes equals, bit for bit, the float32
sum in sorted-input order of each note rendered alone over only its own length (the semantics the score bank rests
on), and rendering such a score in 256- and 777-frame blocks equals one whole render.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from fixture_harness import render_blocks                         # noqa: E402
import score_oracle as S                                           # noqa: E402

SR = S.SR


def ks(rng, i, length):
    src = {"type": "ks", "freq": round(float(np.exp(rng.uniform(np.log(60.0), np.log(1800.0)))), 3),
           "rho": round(float(rng.uniform(0.97, 0.999)), 5), "seed": 100 + i, "crop": [0, length]}
    if i % 3 == 2:                                                  # two-phase, the switch inside the note
        src.update(duration=int(length * rng.uniform(0.2, 0.8)), rho_damping=round(float(rng.uniform(0.5, 0.95)), 4))
    return src


def tone(kind):
    def make(rng, i, length):
        return {"type": kind, "freq": round(float(np.exp(rng.uniform(np.log(80.0), np.log(1500.0)))), 3),
                "amp": round(float(rng.uniform(0.1, 0.5)), 3), "crop": [0, length]}
    return make


def noise(rng, i, length):
    return {"type": "noise", "amp": round(float(rng.uniform(0.1, 0.5)), 3), "seed": 500 + i, "crop": [0, length]}


def array(rng, i, length):
    return {"type": "array", "n": length + 7, "channels": 2, "key": i, "crop": [3, length]}


def score(seed, count, make, total=9000):
    """`count` notes of 50-900 frames spread over about `total` frames."""
    rng = np.random.default_rng(seed)
    notes, at = [], 0
    for i in range(count):
        length = int(rng.integers(50, 901))
        notes.append({"src": make(rng, i, length), "start": at})
        at += int(rng.integers(20, max(21, 2 * total // count)))
    return notes


def mozart():
    """The line of example 19 (K. 333), its first 16 notes: (MIDI pitch, length in 32nds, connected)."""
    line = [(77, 12, 1), (74, 4, 1), (70, 8, 0), (70, 8, 0), (75, 4, 1), (77, 1, 1), (75, 1, 1), (74, 1, 1), (75, 1, 1),
            (79, 8, 0), (69, 8, 0), (None, 4, 0), (69, 4, 0), (72, 4, 1), (70, 4, 0), (74, 4, 1), (72, 4, 1)]
    unit, at, notes = 75, 0, []
    for i, (pitch, n32, connected) in enumerate(line):
        length = n32 * unit
        if pitch is not None:
            sounding = length + 150 if connected else max(50, length // 2)      # plucks ring into the next note
            freq = round(440.0 * 2.0 ** ((pitch - 69) / 12), 4)
            notes.append({"src": {"type": "ks", "freq": freq, "rho": 0.996, "seed": 40 + i, "crop": [0, sounding]},
                          "start": at})
        at += length
    return notes


def cases():
    c = []

    def add(name, kind, mode, notes, compare, **extra):
        c.append(dict({"name": name, "kind": kind, "mode": mode, "notes": notes, "compare": compare, "sr": SR}, **extra))

    add("pluck_overlap", "sequence", "overlap", score(1, 40, ks), "bits")
    add("pluck_non_overlap", "sequence", "non_overlap", score(2, 40, ks), "bits", form="list")
    add("saw_overlap", "sequence", "overlap", score(3, 24, tone("saw")), "tol")
    add("sine_non_overlap", "sequence", "NON_OVERLAP", score(4, 24, tone("sine")), "tol")
    add("noise_overlap", "sequence", "overlap", score(5, 24, noise), "bits", form="list")
    add("array_stereo", "sequence", "overlap", score(6, 24, array), "bits")
    mixed = score(7, 18, ks)
    for i, n in enumerate(mixed):
        if i % 3 == 1:
            n["src"] = tone("sine")(np.random.default_rng(70 + i), i, n["src"]["crop"][1])
    mixed.append({"src": {"type": "sine", "freq": 220.0, "amp": 0.2}, "start": mixed[-1]["start"] + 400})
    add("mixed_unbounded_tail", "sequence", "non_overlap", mixed, "tol")
    auto = score(8, 12, ks)
    for i, n in enumerate(auto):
        n["start"] = None if i % 2 == 0 else n["start"]
    auto[4]["src"]["crop"] = [5, 300]                               # an extent that does not start at 0
    auto[5]["start"] = None
    add("auto_advance", "sequence", "overlap", auto, "bits")
    equal = score(9, 10, ks, total=3000)
    for i in (3, 4, 7):
        equal[i]["start"] = equal[i - 1]["start"]
    add("equal_starts_overlap", "sequence", "overlap", equal, "bits")
    add("equal_starts_non_overlap", "sequence", "non_overlap", json.loads(json.dumps(equal)), "bits")
    negative = score(10, 10, noise, total=3000)
    for n in negative:
        n["start"] -= 1500
    add("negative_starts", "sequence", "non_overlap", negative, "bits")
    add("single_pair", "sequence", "overlap", score(11, 1, ks), "bits", form="bare")
    add("mozart_handbuilt", "handbuilt", None, mozart(), "bits")
    # ---- notes of 3 and 5 channels (arrays: every column its own; plucks and sines: one column repeated), both modes
    def wide(make, channels):
        def made(rng, i, length):
            return dict(make(rng, i, length), channels=channels)
        return made
    for ch, modes in ((3, ("overlap", "non_overlap")), (5, ("overlap",))):
        for mode in modes:
            add(f"ch{ch}_array_{mode}", "sequence", mode, score(20 + ch, 8, wide(array, ch), total=1500), "bits")
            add(f"ch{ch}_pluck_{mode}", "sequence", mode, score(30 + ch, 8, wide(ks, ch), total=1500), "bits")
            add(f"ch{ch}_sine_{mode}", "sequence", mode, score(40 + ch, 8, wide(tone("sine"), ch), total=1500), "tol")
    return c


def refusals(K):
    mk = lambda: K.CropPE(K.SinePE(100.0), 0, 10)                   # noqa: E731
    return {
        "no_pairs": lambda: K.SequencePE(),
        "empty_list": lambda: K.SequencePE([]),
        "not_a_pair": lambda: K.SequencePE((mk(), 0), mk()),
        "triple": lambda: K.SequencePE((mk(), 0, 1), (mk(), 2)),
        "auto_after_infinite": lambda: K.SequencePE((K.SinePE(100.0), 0), (mk(), None)),
        "bad_mode": lambda: K.SequencePE((mk(), 0), (mk(), 5), mode="legato"),
    }


def describe(pe):
    return dict(gen_golden.describe(pe), inner_inputs=[type(i).__name__ for i in pe.inputs()[0].inputs()],
                mode=pe.mode.value if hasattr(pe, "mode") else None,
                pairs=[[type(p).__name__, int(s)] for p, s in getattr(pe, "_pairs", [])])


def conversions(conv):
    midi = list(range(128))
    freqs = [float(f) for f in conv.pitch_to_freq(midi)]
    ratios = [0.25, 0.5, 0.75, 1.0, 1.0594630943592953, 1.5, 2.0, 3.0, 7.3]
    semis = [-24, -12, -7, -1, -0.5, 0, 0.01, 1, 7, 12, 19, 30.5]
    times = [0.0, 1e-4, 0.001, 0.25, 1.0, 2.5, 61.7]
    counts = [0, 1, 64, 1000, 44_100, 48_000, 1_234_567]
    rates = [8000, 44_100, 48_000]
    return {
        "midi": midi, "pitch_to_freq": freqs,
        "freq_to_pitch": [float(v) for v in conv.freq_to_pitch(freqs)],
        "semitones": semis, "semitones_to_ratio": [float(v) for v in conv.semitones_to_ratio(semis)],
        "ratios": ratios, "ratio_to_semitones": [float(v) for v in conv.ratio_to_semitones(ratios)],
        "rates": rates, "seconds": times, "samples": counts,
        "seconds_to_samples": [[float(v) for v in conv.seconds_to_samples(times, r)] for r in rates],
        "samples_to_seconds": [[float(v) for v in conv.samples_to_seconds(counts, r)] for r in rates],
        "scalar_type": type(conv.pitch_to_freq(69)).__name__, "array_dtype": str(conv.pitch_to_freq([69]).dtype),
    }


def main():
    mods = gen_golden.load_reference()
    K = mods["K"]
    mods["config"].set_sample_rate(SR)
    renderer = lambda: mods["null_renderer"].NullRenderer(sample_rate=SR)   # noqa: E731
    arrays, all_cases = {}, cases()
    for case in all_cases:
        pe = build_case_checked(K, case)
        case["pe"] = describe(pe)
        ext = pe.extent()
        first = ext.start if ext.start is not None else 0
        end = ext.end if ext.end is not None else max(n["start"] or 0 for n in case["notes"]) + 1200
        case["patterns"] = S.patterns(first, end)
        case["same_as_whole"] = {}
        outs = {}
        for name, blocks in case["patterns"].items():
            outs[name] = np.concatenate(render_blocks(S.build_case(K, case), SR, blocks, renderer=renderer()))
        arrays[f"{case['name']}/whole"] = outs["whole"]
        probe = dict(case, patterns=case["patterns"], same_as_whole={p: True for p in outs})
        for name in outs:
            if name == "whole":
                continue
            same = np.array_equal(S.expected(probe, name, _Files(arrays)), outs[name])
            case["same_as_whole"][name] = bool(same)
            if not same:
                arrays[f"{case['name']}/{name}"] = outs[name]
        plucks_only = all(n["src"]["type"] == "ks" for n in case["notes"])
        if plucks_only:
            assert case["same_as_whole"]["blocks_256"] and case["same_as_whole"]["blocks_777"], case["name"]
        if plucks_only and case["kind"] == "sequence":
            check_sum_of_notes(K, case, pe, renderer, outs["whole"])
        print(f"{case['name']}: {outs['whole'].shape} {case['same_as_whole']}", flush=True)
    errors = {}
    for name, make in refusals(K).items():
        try:
            make()
        except Exception as exc:                                    # noqa: BLE001
            errors[name] = {"type": type(exc).__name__, "text": str(exc)}
        else:
            raise AssertionError(f"{name}: the reference accepted it")
    gen_golden.write_fixture("score", {"numpy": np.__version__, "sr": SR, "cases": all_cases, "refused": errors,
                                       "conversions": conversions(mods["conversions"])}, arrays)


class _Files(dict):
    files = property(lambda self: list(self.keys()))


def build_case_checked(K, case):
    pe = S.build_case(K, case)
    assert pe.channel_count() in (1, 2, 3, 5), case["name"]
    return pe


def check_sum_of_notes(K, case, pe, renderer, whole):
    """The reference's SequencePE == the float32 sum, in sorted-input order, of each note rendered alone over only its
    own length (OVERLAP) or up to the next start (NON_OVERLAP)."""
    w0, wn = case["patterns"]["whole"][0]
    want = np.zeros((wn, whole.shape[1]), dtype=np.float32)
    pairs = pe._pairs
    fresh = S.build_case(K, case)._pairs
    for k, ((_, start), (src, _)) in enumerate(zip(pairs, fresh)):
        ext = src.extent()
        length = ext.end - ext.start
        if pe.mode.value == "non_overlap" and k + 1 < len(pairs):
            length = min(length, max(0, pairs[k + 1][1] - start))
        if length <= 0:
            continue
        alone = render_blocks(src, SR, [[ext.start, length]], renderer=renderer())[0]
        lo = start + ext.start - w0
        want[lo:lo + length] = want[lo:lo + length] + alone
    assert np.array_equal(want, whole), f"{case['name']}: not the ordered sum of its notes"


if __name__ == "__main__":
    main()
