"""
Fixtures for panned voices under a MixPE (voice_bank._PanNode): render the cases below through the reference
implementation (a started NullRenderer graph, the caller's blocks) and write tests/golden/panned_mix_cases.json +
tests/golden/panned_mix.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_panned_mix.py
The npz holds data only: per case the float32 samples (frames, 2) of its blocks ("<name>").  The json holds the graph
SPECs (tests/pan_cases.py: the graphs the twin-render and trace tests use), the blocks and "compare": "fuzz" -- the
graphs hold oscillators and filters, so each block is held to REL_TOL * its peak + ABS_FLOOR
(tests/fixture_harness.check_case).

Cases, five voices each, three contiguous blocks of 1 024 frames at 48 kHz:
    panned_mix_lfo      BiquadPE(BlitSawPE) under SpatialLinear(azimuth=SinePE): every voice swings past +-90 degrees
    panned_mix_readme   README.md's voice under SpatialConstantPower(azimuth=a_i): scalar azimuths, two of them clipped

Checked while generating, against the reference alone: every case's peak is above 0.1 and its two channels differ.
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden                                     # noqa: E402
from oracle.gen_golden import render_reference, write_fixture      # noqa: E402
from oracle.golden_cases import blocks_contig                      # noqa: E402
import pan_cases                                                   # noqa: E402

MIN_PEAK = 0.1


def cases():
    blocks = blocks_contig(0, [1024] * 3)
    return [{"name": f"panned_mix_{kind}", "sr": pan_cases.SR, "graph": pan_cases.mix(kind), "blocks": blocks,
             "compare": "fuzz"} for kind in ("lfo", "readme")]


def main():
    mods = gen_golden.load_reference()
    arrays, all_cases = {}, cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe, _ = render_reference(case, mods, ())
        flat = np.concatenate(outs)
        assert flat.dtype == np.float32 and flat.shape == (3 * 1024, 2), (case["name"], flat.dtype, flat.shape)
        peak = float(np.max(np.abs(flat)))
        assert np.all(np.isfinite(flat)) and peak > MIN_PEAK, f"{case['name']}: peak {peak:g}"
        apart = float(np.max(np.abs(flat[:, 0] - flat[:, 1])))
        assert apart > 0.01 * peak, f"{case['name']}: the channels differ by {apart:g} at most"
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        arrays[case["name"]] = flat
        print(f"{case['name']}: {flat.shape} peak {peak:.4f}, channels apart by up to {apart:.4f}", flush=True)
    write_fixture("panned_mix", {"cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
