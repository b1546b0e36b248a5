"""
Fixtures for PortamentoPE: render the reference's PortamentoPE (a started NullRenderer graph, the caller's requests) on
the note tables below and write tests/golden/portamento_cases.json + tests/golden/portamento.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_portamento.py

The reference's PortamentoPE hands `channels=` to its SequencePE, which does not take it, so two or more notes raise
TypeError.  The generator wraps SequencePE.__init__ in this process to swallow that one keyword (three lines below, the
reference's files are not touched); everything rendered is the reference's own composition of PiecewisePE, CropPE,
DelayPE and MixPE.

The npz holds data only: per case the float32 samples of its requests, concatenated ("<name>"), per departure the
reference's block ("departure/<name>").  The json holds the tables, the parameters, the requests, what the reference
says about each PE (repr, purity, channels), its four validation messages and the departures.

Checked while generating, against the reference alone:
  * the numpy restatement of the closed form (tests/portamento_oracle.py) reproduces every request of every case bit for
    bit;
  * every request of a case with three or more notes starts at or after the second note's start;
  * the two departures are exactly what the json records: in each departure's request the reference renders 0.0 over
    "zero_frames" (a range of the request's frames), where the closed form holds the first pitch, and the two agree bit
    for bit on every other frame.
"""

from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import write_fixture                       # noqa: E402
import portamento_oracle as PO                                    # noqa: E402

SR = 44100


def cases():
    c = []

    def add(name, notes, requests, max_ramp_seconds=0.1, ramp_fraction=0.3, channels=1, sr=SR):
        c.append({"name": name, "sr": sr, "notes": [list(n) for n in notes], "max_ramp_seconds": max_ramp_seconds,
                  "ramp_fraction": ramp_fraction, "channels": channels, "requests": [list(r) for r in requests]})

    # one note: its pitch everywhere, before the note as well
    add("one_note", [(69.0, 500, 1000)], [[-200, 100], [0, 1], [400, 300], [2000, 64]])
    # two notes, one ramp (at 1000, 300 frames): requests that begin at `at`, `at + len - 1` and `at + len`
    add("two_notes", [(69.0, 0, 1000), (73.0, 1000, 1000)],
        [[-500, 200], [900, 400], [1000, 1], [1299, 1], [1300, 1], [1000, 300], [1299, 2], [5000, 100]])
    # the docstring's example
    add("three_abutting", [(69.0, 0, 1000), (73.0, 1000, 1000), (76.0, 2000, 1000)],
        [[1000, 1500], [2000, 1], [2299, 1], [2300, 1], [1000, 4000], [2150, 65]])
    # five notes, up and down, pitches that float32 does not hold
    add("five_notes", [(76.1, 0, 800), (72.3, 800, 800), (69.0, 1600, 800), (71.7, 2400, 800), (60.25, 3200, 800)],
        [[800, 3500], [1600, 1], [1839, 2], [3200, 240], [3440, 63]])
    add("descending", [(72.0, 0, 900), (60.0, 900, 900), (48.5, 1800, 900)], [[900, 2000], [1170, 1], [2069, 2]])
    # gaps: the previous pitch is held through the gap
    add("gaps", [(60.0, 0, 500), (64.0, 1000, 500), (67.0, 3000, 200)], [[1000, 3000], [3059, 3]])
    # an overlap: the third note begins 200 frames into the 900-frame glide to the second and cuts it
    add("overlap_cut", [(60.0, 0, 1500), (64.0, 1000, 3000), (67.0, 1200, 1000)], [[1000, 600], [1199, 2], [1200, 300]])
    # a note of duration 0: a ramp of one frame
    add("zero_duration", [(60.0, 0, 100), (72.0, 500, 0), (48.0, 900, 400)], [[500, 3], [500, 1], [501, 1], [500, 600]])
    add("fraction_0", [(60.0, 0, 1000), (67.0, 1000, 1000), (62.0, 2000, 1000)], [[1000, 1200], [1000, 2]],
        ramp_fraction=0.0)
    add("fraction_1", [(60.0, 0, 1000), (67.0, 1000, 1000), (62.0, 2000, 1500)], [[1000, 2600], [1999, 2], [3499, 2]],
        ramp_fraction=1.0)
    add("max_ramp_0", [(60.0, 0, 1000), (67.0, 1000, 1000), (62.0, 2000, 1000)], [[1000, 1200], [2000, 2]],
        max_ramp_seconds=0.0)
    add("unsorted", [(67.0, 2000, 700), (60.0, 0, 1000), (71.5, 2700, 600), (64.0, 1000, 1000)], [[1000, 2400]])
    add("two_channels", [(69.0, 0, 1000), (73.0, 1000, 1000), (76.0, 2000, 1000)], [[1000, 1400], [2299, 2]], channels=2)
    add("three_channels", [(64.0, 100, 700), (57.5, 800, 900)], [[-100, 1300], [1069, 2]], channels=3)
    # max_ramp_seconds binds: 441 frames at 44 100, 480 at 48 000, under notes that would allow 900
    for sr in (44100, 48000):
        add(f"max_ramp_binds_{sr}", [(60.0, 0, 3000), (72.0, 3000, 3000), (65.0, 6000, 3000)],
            [[3000, 600], [3440, 2], [3479, 2], [6000, 500]], max_ramp_seconds=0.01, sr=sr)
    return c


def departures():
    """Where the reference, patched as above, leaves its own docstring ("infinite extent", "holds the first note's pitch
    for all times before the first note"); `zero_frames`: the frames of the request that it renders as 0."""
    abutting = [[69.0, 0, 1000], [73.0, 1000, 1000], [76.0, 2000, 1000]]
    shared = [[60.0, 0, 1000], [64.0, 1000, 1000], [67.0, 1000, 1000]]

    def dep(name, why, notes, request, zero_frames):
        return {"name": name, "why": why, "sr": SR, "notes": notes, "max_ramp_seconds": 0.1, "ramp_fraction": 0.3,
                "channels": 1, "request": request, "zero_frames": zero_frames}

    before = "three or more notes: a request wholly before the second note's start is outside the reference's extent"
    return [
        dep("before_second_note", before, abutting, [-200, 100], [0, 100]),
        dep("last_frame_before_second_note", before, abutting, [999, 1], [0, 1]),
        dep("straddling_second_note", "the same table, a request that straddles the second note's start: no departure",
            abutting, [900, 101], [0, 0]),
        dep("shared_start", "the second and third notes share a start: the first ramp's crop has no length, and the "
            "frames before that start render as 0 in a straddling request too", shared, [-500, 2000], [0, 1500]),
    ]


def reference_classes():
    mods = gen_golden.load_reference()
    sequence = importlib.import_module("pygmu2.sequence_pe")
    portamento = importlib.import_module("pygmu2.portamento_pe")
    init = sequence.SequencePE.__init__

    def init_without_channels(self, *pairs, channels=None, **kwargs):
        init(self, *pairs, **kwargs)
    sequence.SequencePE.__init__ = init_without_channels
    return mods, portamento.PortamentoPE


def render(mods, PortamentoPE, case, requests):
    mods["config"].set_sample_rate(case["sr"])
    pe = PO.build(types.SimpleNamespace(PortamentoPE=PortamentoPE), case)
    renderer = mods["null_renderer"].NullRenderer(sample_rate=case["sr"])
    renderer.set_source(pe)
    renderer.start()
    outs = []
    for s, n in requests:
        data = pe.render(int(s), int(n)).data
        assert data.dtype == np.float32 and data.shape == (n, case["channels"]), (case["name"], data.dtype, data.shape)
        outs.append(np.ascontiguousarray(data))
    return pe, outs


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def main():
    mods, PortamentoPE = reference_classes()
    arrays, doc = {}, {"cases": cases(), "departures": departures(), "errors": {}}
    for case in doc["cases"]:
        tab = PO.case_table(case)
        second = sorted(n[1] for n in case["notes"])[1] if len(case["notes"]) >= 3 else None
        pe, outs = render(mods, PortamentoPE, case, case["requests"])
        for (s, n), got in zip(case["requests"], outs):
            assert second is None or s >= second, f"{case['name']}: request {s} begins before the second note"
            assert same_bits(got, PO.line(tab, s, n, case["channels"])), \
                f"{case['name']} [{s}, +{n}): the closed form is not what the reference renders"
        case["reference"] = {"repr": repr(pe), "pure": bool(pe.is_pure()), "channels": pe.channel_count(),
                             "notes": [list(n) for n in pe.notes]}
        arrays[case["name"]] = np.concatenate(outs)
        print(f"{case['name']}: {len(outs)} requests, {arrays[case['name']].shape[0]} frames, "
              f"{tab[0].shape[0]} ramp(s) of {tab[1].tolist()} frames", flush=True)
    for d in doc["departures"]:
        s, n = d["request"]
        _, (got,) = render(mods, PortamentoPE, d, [d["request"]])
        want = PO.line(PO.case_table(d), s, n)
        a, b = d["zero_frames"]
        keep = np.ones(n, bool)
        keep[a:b] = False
        assert not np.any(got[a:b]) and np.all(want[a:b] == np.float32(sorted(d["notes"], key=lambda x: x[1])[0][0]))
        assert same_bits(got[keep], want[keep]), f"{d['name']}: the departure is wider than recorded"
        arrays[f"departure/{d['name']}"] = got
        print(f"departure {d['name']}: the reference renders 0 over frames {a}..{b} of [{s}, +{n})")
    refusals = {"empty": lambda: PortamentoPE([]),
                "negative_max_ramp": lambda: PortamentoPE([(60.0, 0, 10)], max_ramp_seconds=-0.5),
                "fraction_above_1": lambda: PortamentoPE([(60.0, 0, 10)], ramp_fraction=1.5),
                "fraction_below_0": lambda: PortamentoPE([(60.0, 0, 10)], ramp_fraction=-0.25),
                "no_channels": lambda: PortamentoPE([(60.0, 0, 10)], channels=0)}
    for key, make in refusals.items():
        try:
            make()
            raise AssertionError(f"{key}: the reference accepts it")
        except ValueError as e:
            doc["errors"][key] = str(e)
    write_fixture(PO.FIXTURE, doc, arrays)


if __name__ == "__main__":
    main()
