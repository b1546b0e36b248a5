"""
Fixtures for modulated-sine voices under a MixPE (voice_bank._SineModNode): render the cases below through the reference
implementation (a started NullRenderer graph, the caller's blocks) and write tests/golden/fm_voices_cases.json +
tests/golden/fm_voices.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_fm_voices.py
The npz holds data only: per case the float32 samples (frames, 1) of its blocks ("<name>").  The json holds the graph
SPECs (tests/fm_cases.py: the graphs the twin-render tests use), the blocks, the one lifecycle op and "compare": "fuzz" --
the graphs hold oscillators, so each block is held to REL_TOL * its peak + ABS_FLOOR (tests/fixture_harness.check_case).

Cases, five voices each at 48 kHz: contiguous blocks of 1 024, 3 077 and 1 024 frames (the reference enforces contiguity on
a PE that is not pure), renderer stop + start, then 2 049 and 1 024 frames from frame 0 -- 8 198 frames per case.
    fm_voices_fm       two-operator FM
    fm_voices_am_pm    an amplitude PE and a phase PE: the phase is carried into the next block and added again
    fm_voices_nested   the modulator is itself an FM voice
    fm_voices_bell     an FM voice under GainPE with an AdsrTriggeredPE(PeriodicTrigger) envelope

Checked while generating: every case's peak is above 0.1; the stop + start cleared the phase (block 3 begins as block 0
did); and the project's CPU restatement (oracle/graph_eval.py) is within the fixture's rule of the reference in every
block of every case -- a case that is not has too large a modulation index for the rule (tests/fm_cases.py), not too
tight a rule.
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden, graph_eval                          # noqa: E402
from oracle.gen_golden import render_reference, write_fixture      # noqa: E402
from oracle.golden_cases import blocks_contig                      # noqa: E402
import fixture_harness as H                                        # noqa: E402
import fm_cases                                                    # noqa: E402

MIN_PEAK = 0.1
MAX_FRAMES = 10_000
RESTART_AT = 3


def cases():
    blocks = blocks_contig(0, [1024, 3077, 1024]) + blocks_contig(0, [2049, 1024])
    assert sum(n for _, n in blocks) <= MAX_FRAMES
    return [{"name": f"fm_voices_{kind}", "sr": fm_cases.SR, "graph": fm_cases.mix(kind), "blocks": blocks,
             "ops": {str(RESTART_AT): "restart"}, "compare": "fuzz"} for kind in fm_cases.KINDS]


def restated(case):
    """The case through oracle/graph_eval.py; stop + start is the graph's reset."""
    g = graph_eval.make_node(case["graph"], case["sr"])
    outs = []
    for i, (s, n) in enumerate(case["blocks"]):
        if case["ops"].get(str(i)) == "restart":
            g.reset()
        outs.append(np.asarray(g.render(int(s), int(n)), dtype=np.float32))
    return outs


def main():
    mods = gen_golden.load_reference()
    arrays, all_cases = {}, cases()
    for case in all_cases:
        mods["config"].set_sample_rate(case["sr"])
        outs, pe, _ = render_reference(case, mods, ())
        flat = np.concatenate(outs)
        frames = sum(n for _, n in case["blocks"])
        assert flat.dtype == np.float32 and flat.shape == (frames, 1), (case["name"], flat.dtype, flat.shape)
        peak = float(np.max(np.abs(flat)))
        assert np.all(np.isfinite(flat)) and peak > MIN_PEAK, f"{case['name']}: peak {peak:g}"
        assert np.array_equal(outs[RESTART_AT][:1024], outs[0]), f"{case['name']}: stop + start did not clear the phase"
        worst = 0.0
        for i, (got, want) in enumerate(zip(restated(case), outs)):
            block_peak = float(np.max(np.abs(want)))
            err = H.max_err(got, want)
            worst = max(worst, err / (H.REL_TOL * block_peak + H.ABS_FLOOR))
            assert H.within("fuzz", got, want, block_peak), \
                f"{case['name']} block {i}: the restatement is off by {err:.3e} (peak {block_peak:.3e}): reduce the index"
        ext = pe.extent()
        case["extent"] = [ext.start, ext.end]
        arrays[case["name"]] = flat
        print(f"{case['name']}: {flat.shape} peak {peak:.4f}, restatement at {worst:.3e} of the rule", flush=True)
    write_fixture("fm_voices", {"cases": all_cases}, arrays)


if __name__ == "__main__":
    main()
