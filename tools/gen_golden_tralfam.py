"""
Fixtures for TralfamPE, SlicePE and SetExtentPE: render the cases below through the reference implementation and write
tests/golden/tralfam_cases.json + tests/golden/tralfam.npz.

Needs the reference package (oracle.gen_golden.load_reference; tralfam_pe, slice_pe, set_extent_pe and noise_pe are
imported next to it) and numpy >= 2: the reference's forward transform is complex64 there and `normalize_peak / peak` a
float32 quotient (NEP 50); the version used is recorded in the json.  Run from the repository root:
    python tools/gen_golden_tralfam.py
The npz holds data only: short input signals ("in_<name>") and per case what tests/tralfam_oracle.stored_of keeps of the
reference's blocks ("<name>") -- every sample of a "full" case, the sampled frames of a "sampled" one (first and last
1024 frames, 1024 around N/2 and around the peak, every ceil(N/8192)-th frame).  The json holds the cases (source
signal, graph shape, seed, normalize_peak, blocks), the reference's extent / repr / purity / channel count / inputs of
the PE under test, and for a TralfamPE case the float32 peak of the whole result and where it sits.  Long inputs are
rebuilt from the json by integer arithmetic (tralfam_oracle.make_signal); the stereo file case reads
tests/golden/kemar/H0e030a.wav, which the reference side is handed as an ArrayPE of the same int16 / 32768 samples (its
own WavReaderPE needs the absent soundfile).

Checked while generating, against the reference alone: the float64 restatement (tests/tralfam_oracle.py) gives every
TralfamPE case within fixture_harness.PEAK_BOUND * peak of the case, every SetExtentPE case and every SlicePE case without fades bit
for bit, and SlicePE with fades within the GainPE class; a silent case is exactly zero.
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from fixture_harness import within                                # noqa: E402
import tralfam_oracle as T                                         # noqa: E402

SR = 48000
SEEDS = T.SEEDS
WAV = "H0e030a.wav"


def noise(n, channels=1):
    return {"kind": "noise_decay", "n": n, "channels": channels}


def whole(n):
    return [[0, n]]


def blocks_of(first, last, step):
    return [[s, step] for s in range(first, last, step)]


def short_inputs():
    """Signals that need a transcendental function: stored, not rebuilt."""
    i = np.arange(1000, dtype=np.float64)
    j = np.arange(4096, dtype=np.float64)
    return {
        "in_sine_off_1000": (0.5 * np.sin(2 * np.pi * 37.37 * i / 1000)).astype(np.float32),
        "in_sine_on_1000": (0.5 * np.sin(2 * np.pi * 40.0 * i / 1000)).astype(np.float32),
        "in_sine_off_4096": (0.7 * np.sin(2 * np.pi * 123.456 * j / 4096 + 0.3)).astype(np.float32),
        "in_sine_on_4096": (0.7 * np.cos(2 * np.pi * 256.0 * j / 4096)).astype(np.float32),
    }


def cases():
    c = []

    def add(name, graph, source, blocks, **extra):
        n = sum(k for _, k in blocks)
        c.append(dict({"name": name, "sr": SR, "graph": graph, "source": source, "blocks": blocks,
                       "store": "full" if n <= T.FULL_STORE_LIMIT else "sampled"}, **extra))

    # ---- every length once: hashed noise with a decay, the seeds in turn, with and without normalize_peak
    lengths = (1, 2, 3, 7, 128, 1000, 4096, 65_536, 4097, 16_964, 105_164, 99_991)
    for i, n in enumerate(lengths):
        add(f"len_{n}", "plain", noise(n), whole(n), seed=SEEDS[i % len(SEEDS)],
            normalize_peak=None if i % 2 == 0 else 0.5)
    add("len_16964_normalized", "plain", noise(16_964), whole(16_964), seed=SEEDS[2], normalize_peak=0.9)
    add("len_132300_stereo", "plain", {"kind": "stereo60", "n": 132_300, "channels": 2}, whole(132_300), seed=SEEDS[1],
        normalize_peak=None)
    add("len_156168_stereo", "plain", noise(156_168, 2), whole(156_168), seed=SEEDS[0], normalize_peak=0.8)
    add("len_1048577", "plain", noise(1_048_577), whole(1_048_577), seed=SEEDS[2], normalize_peak=None)
    add("len_2097151", "plain", noise(2 ** 21 - 1), whole(2 ** 21 - 1), seed=SEEDS[3], normalize_peak=0.5)
    add("len_2097152", "plain", noise(2 ** 21), whole(2 ** 21), seed=SEEDS[4], normalize_peak=None)

    # ---- the signal kinds, with and without normalize_peak
    kinds = [("sine_off", {"kind": "array", "name": "in_sine_off_1000"}),
             ("sine_on", {"kind": "array", "name": "in_sine_on_1000"}),
             ("dirac", {"kind": "dirac", "n": 1000}), ("dc", {"kind": "dc", "n": 1000}),
             ("ramp", {"kind": "ramp", "n": 1000}), ("silence", {"kind": "silence", "n": 1000}),
             ("stereo60", {"kind": "stereo60", "n": 1000, "channels": 2}),
             ("stereo_dirac_dc", {"kind": "dirac", "n": 999, "channels": 2})]
    for i, (label, src) in enumerate(kinds):
        n = src.get("n", 1000)
        add(f"kind_{label}", "plain", src, whole(n), seed=SEEDS[i % len(SEEDS)], normalize_peak=None)
        add(f"kind_{label}_normalized", "plain", src, whole(n), seed=SEEDS[(i + 1) % len(SEEDS)], normalize_peak=0.25)
    add("kind_sine_off_4096", "plain", {"kind": "array", "name": "in_sine_off_4096"}, whole(4096), seed=7,
        normalize_peak=None)
    add("kind_sine_on_4096", "plain", {"kind": "array", "name": "in_sine_on_4096"}, whole(4096), seed=8,
        normalize_peak=1.0)
    add("kind_silence_long", "plain", {"kind": "silence", "n": 16_964}, whole(16_964), seed=3, normalize_peak=0.5)
    add("kind_ramp_long", "plain", {"kind": "ramp", "n": 20_000}, whole(20_000), seed=4, normalize_peak=None)
    add("kind_dirac_long", "plain", {"kind": "dirac", "n": 10_007}, whole(10_007), seed=5, normalize_peak=0.5)
    add("wav_stereo", "plain", {"kind": "wav", "file": WAV}, whole(128), seed=9, normalize_peak=None)
    add("seed_none_shape", "plain", noise(64), [[-8, 4]], seed=None, normalize_peak=None)   # outside the extent: zeros

    # ---- render patterns
    add("blocks_1000", "plain", noise(3500), blocks_of(-2000, 6000, 1000), seed=SEEDS[1], normalize_peak=0.7)
    add("delay_positive", "delay", noise(1500), blocks_of(0, 3000, 1000), delay=700, seed=SEEDS[2], normalize_peak=None)
    add("delay_negative", "delay", noise(2500), blocks_of(-2000, 2000, 1000), delay=-1300, seed=SEEDS[3],
        normalize_peak=None)
    add("same_block_twice", "plain", noise(2000), [[500, 1000], [500, 1000], [1900, 200], [1900, 200]], seed=SEEDS[4],
        normalize_peak=None)
    add("loop_4", "loop", noise(777), blocks_of(0, 4000, 1000), count=4, seed=SEEDS[0], normalize_peak=0.5)
    add("example_slice_set_extent", "example", noise(6000), [[0, 2000 + 2 * SR]], start=500, duration=2000,
        fade_in_seconds=0.005, fade_out_seconds=0.01, seed=SEEDS[1], normalize_peak=0.5)
    add("example_wav", "example", {"kind": "wav", "file": WAV}, blocks_of(-1000, 3000, 1000), sr=1000, start=16,
        duration=96, seed=SEEDS[2], normalize_peak=None)
    add("noise_crop_then_pull", "noise_crop", {"kind": "noise", "n": 2048}, [[0, 2048], [1000, 2048]], noise_seed=7,
        after=256, seed=SEEDS[1], normalize_peak=None)

    # ---- SlicePE alone (sr 1000: fades in frames = milliseconds)
    fades = {"no_fade": (None, None), "fade_in": (0.05, None), "fade_out": (None, 0.08), "both": (0.05, 0.08),
             "longer_than_slice": (1.0, 2.0)}
    for label, (fi, fo) in fades.items():
        add(f"slice_{label}", "slice", noise(600, 2), [[-100, 500], [400, 100], [0, 300]], sr=1000, start=150,
            duration=300, fade_in_seconds=fi, fade_out_seconds=fo)
    add("slice_zero_duration", "slice", noise(600), [[-10, 50]], sr=1000, start=100, duration=0,
        fade_in_seconds=0.05, fade_out_seconds=0.05)
    add("slice_past_the_source", "slice", noise(600), [[-10, 400]], sr=1000, start=500, duration=300,
        fade_in_seconds=None, fade_out_seconds=0.1)

    # ---- SetExtentPE alone: the source is [0, 300)
    for mode in ("zero", "hold_first", "hold_last", "hold_both"):
        add(f"set_extent_{mode}", "set_extent", noise(300, 2), [[-100, 700], [0, 64], [40, 20], [280, 40], [600, 10]],
            start=50, duration=200, extend_mode=mode)
        add(f"set_extent_longer_{mode}", "set_extent", noise(300), [[-100, 700], [440, 20]], start=-20, duration=470,
            extend_mode=mode)
    add("set_extent_open_start", "set_extent", noise(300), [[-100, 700], [100, 50], [190, 20]], start=None, duration=200,
        extend_mode="hold_both")
    add("set_extent_open_end", "set_extent", noise(300), [[-100, 700], [90, 20]], start=100, duration=None,
        extend_mode="hold_both")
    add("set_extent_open_both", "set_extent", noise(300), [[-100, 700]], start=None, duration=None, extend_mode="zero")

    # ---- 3, 4, 5 and 8 channels (every column its own noise): a float4 straddles frames at 3, lies inside one at 5, a
    # frame is one or two float4s at 4 and 8.  499 frames: no power of two, the arbitrary-length transform per channel
    for ch in (3, 4, 5, 8):
        add(f"ch{ch}_tralfam_499", "plain", noise(499, ch), whole(499), seed=SEEDS[ch % len(SEEDS)],
            normalize_peak=None if ch % 2 else 0.5)
        add(f"ch{ch}_slice_both", "slice", noise(600, ch), [[-100, 500]], sr=1000, start=150, duration=300,
            fade_in_seconds=0.05, fade_out_seconds=0.08)
        add(f"ch{ch}_set_extent_hold_both", "set_extent", noise(300, ch), [[-100, 300], [200, 200]], start=50, duration=200,
            extend_mode="hold_both")
    for case in c:
        if case["graph"] in ("slice", "set_extent"):
            faded = case["graph"] == "slice" and case["duration"] > 0 and (
                (case.get("fade_in_seconds") or 0) > 0 or (case.get("fade_out_seconds") or 0) > 0)
            case["compare"] = "gain" if faded else "bits"
        else:
            case["compare"] = "peak"
    return c


def main():
    assert int(np.__version__.split(".")[0]) >= 2, f"numpy {np.__version__}: the fixtures need numpy >= 2 (NEP 50)"
    mods = gen_golden.load_reference()
    K = mods["K"]
    K.wav = lambda name: K.ArrayPE(T.read_wav(name))      # the reference's own WavReaderPE needs the absent soundfile
    arrays = short_inputs()
    all_cases = cases()
    worst = 0.0
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe = T.render_case(case, K, arrays)
        case["pe"] = gen_golden.describe(pe)
        if case["compare"] == "peak":
            whole_out = np.concatenate(outs[:len(case["blocks"])])
            peak = float(np.max(np.abs(whole_out))) if whole_out.size else 0.0
            flat = np.abs(whole_out).max(axis=1) if whole_out.size else np.zeros(0)
            case["peak"] = peak
            case["peak_at"] = int(np.argmax(flat)) if flat.size else 0
        else:
            peak = max(float(np.max(np.abs(o))) if o.size else 0.0 for o in outs)
        restated = T.restate_case(case, arrays)
        assert len(restated) == len(outs), case["name"]
        for i, (a, b) in enumerate(zip(outs, restated)):
            assert within(case["compare"], b, a, peak, silent="zero"), f"{case['name']}: the restatement differs from the reference in block {i}"
            if case["compare"] == "peak" and peak > 0 and a.size:
                worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) / peak)
        if case["source"]["kind"] == "silence":
            assert all(not np.any(o) for o in outs), f"{case['name']}: silence in, something out"
        arrays[case["name"]] = T.stored_of(case, outs)
        print(f"{case['name']}: {arrays[case['name']].shape} {case['compare']} {case['store']}", flush=True)
    print(f"largest distance reference <-> float64 restatement: {worst:.3e} x peak")
    gen_golden.write_fixture("tralfam", {"numpy": np.__version__, "cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
