"""
Fixtures for RandomSelectPE: render the cases below through the reference implementation (a started NullRenderer graph,
the caller's blocks) and write tests/golden/random_select_cases.json + tests/golden/random_select.npz.

Needs the reference package (oracle.gen_golden.load_reference); run from the repository root:
    python tools/gen_golden_random_select.py
The npz holds data only: per case and block pattern the float32 samples of its blocks, concatenated
("<name>/<pattern>"); a pattern whose samples equal the one-block render's is not stored twice (the json says so under
"same_as_whole").  The json holds the graphs (the vocabulary of tests/random_select_oracle.build), the blocks of every
pattern, the lifecycle "ops" (tests/fixture_harness.render_blocks: "restart" = stop + start of the renderer, "reset" = the
RandomSelectPE's reset_state()), how each case is compared -- "bits", or "float": per block REL_TOL * peak +
SCORE_ABS_FLOOR (tests/fixture_harness.py), the bar tests/test_gpu_score.py holds oscillator sources to -- and what the
reference says about the class: its validation errors, inputs(), is_pure(), extent and channel count.

Checked while generating, against the reference alone: every sample is finite, and every "float" case has a peak above
0.05 -- a bar relative to a silent case is no bar.
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
import fixture_harness as H                                       # noqa: E402
import random_select_oracle as R                                  # noqa: E402

SR = R.SR
N = 3000

# An event on frame 0 of a 250-frame block (500) and on the last frame of one (749), two adjacent (1000, 1001), an event
# in a block of one frame of the ragged pattern (451, 1063), a +2, a -1 (no event), 300 frames of silence before the
# first, blocks without an event ([0, 250), [2000, 2250)), gaps from 1 to 399 frames, an event on the last frame.
IRREGULAR = {"t": "atrig", "n": N, "events": [
    [300, 1], [451, 1], [500, 1], [749, 1], [1000, 1], [1001, 1], [1063, 1], [1300, 2], [1400, -1], [1450, 1], [1460, 1],
    [1700, 1], [1990, 1], [2250, 1], [2600, 1], [2620, 1], [2999, 1]]}


def ptrig(hz):
    return {"t": "ptrig", "hz": hz}


def slices(ch):
    """Three slices of 30, 90 and 200 frames: each shorter than some gaps of IRREGULAR and longer than others."""
    return [{"t": "slice", "src": {"t": "array", "n": 700, "ch": ch, "key": 3 + k}, "start": start, "dur": dur}
            for k, (start, dur) in enumerate(((5, 30), (100, 90), (333, 200)))]


def pitch(p):
    return 440.0 * 2.0 ** ((p - 69) / 12.0)


def cases():
    c = []

    def add(name, graph, compare, only=None, **extra):
        pats = R.patterns(N)
        if only:
            pats = {only: pats[only]}
        c.append(dict({"name": name, "sr": SR, "graph": graph, "compare": compare, "patterns": pats}, **extra))

    def rsel(trigger, inputs, weights=None, seed=1234):
        return {"t": "rsel", "trigger": trigger, "inputs": inputs, "weights": weights, "seed": seed}

    consts = [{"t": "const", "v": v} for v in (0.25, -0.5, 0.75, 1.0)]
    add("const4_weighted", rsel(ptrig(100.0), consts, [0.1, 0.4, 0.2, 0.3]), "bits")
    for ch in (1, 2, 3):
        add(f"slices_{ch}ch", rsel(IRREGULAR, slices(ch), None, seed=7 + ch), "bits")
    sine_weights = [0.1, 0.4, 0.2, 0.3, 0.4, 0.4]
    sines = [{"t": "sine", "f": pitch(p), "amp": 0.3} for p in (55, 57, 62, 64, 69, 71)]
    add("demo1_weighted_sines", rsel(ptrig(25.0), sines, sine_weights), "float")
    freqs = [{"t": "const", "v": pitch(p)} for p in (55, 57, 62, 64, 69, 71)]
    add("demo2_one_oscillator", {"t": "sine", "f": rsel(ptrig(25.0), freqs, [0.1, 0.4, 0.2, 0.3, 0.4, 0.1]), "amp": 0.3},
        "float")
    add("irregular_mixed", rsel(IRREGULAR, [{"t": "sine", "f": 300.0, "amp": 0.5}, {"t": "const", "v": 0.5},
                                            slices(1)[2]], [0.5, 0.2, 0.3], seed=99), "float")
    # stop + start before block 4 (the sequence of draws goes on, the running stretch is forgotten), reset_state()
    # before block 8 (one draw, silence until the next event)
    add("lifecycle_ops", rsel(ptrig(30.0), slices(2), None, seed=5), "bits", only="equal",
        ops={"4": "restart", "8": "reset"})
    # candidates that carry state: the composed path
    saws = [{"t": "saw", "f": 220.0, "amp": 0.5}, {"t": "saw", "f": 330.0, "amp": 0.4}]
    add("stateful_saws", rsel(ptrig(50.0), saws, None, seed=11), "float")
    return c


def facts(K):
    """What the reference says about the class, for tests/test_random_select_host.py."""
    trig = K.PeriodicTrigger(hz=10.0)
    a, b = K.ConstantPE(1.0), K.ConstantPE(2.0, channels=2)
    pe = K.RandomSelectPE(trig, [a, K.ConstantPE(3.0)], weights=[1, 2], seed=1)
    refusals = {"no_inputs": lambda: K.RandomSelectPE(trig, []),
                "weights_length": lambda: K.RandomSelectPE(trig, [a, b], weights=[1.0]),
                "channel_mismatch": lambda: pe.resolve_channel_count([1, 2, 2, 3]),
                "no_audio_inputs": lambda: pe.resolve_channel_count([1])}
    errors = {}
    for key, make in refusals.items():
        try:
            make()
            raise AssertionError(f"{key}: the reference accepts it")
        except ValueError as e:
            errors[key] = {"type": type(e).__name__, "text": str(e)}
    ext = pe.extent()
    return {"errors": errors, "inputs": [type(i).__name__ for i in pe.inputs()], "pure": bool(pe.is_pure()),
            "extent": [ext.start, ext.end], "channels": pe.channel_count(),
            "resolve": {"[1, 2, 2]": pe.resolve_channel_count([1, 2, 2])}}


def main():
    mods = gen_golden.load_reference()
    K = mods["K"]
    for name in ("random_select_pe", "slice_pe"):
        mod = importlib.import_module(f"pygmu2.{name}")
        for attr in ("RandomSelectPE", "SlicePE"):
            if hasattr(mod, attr):
                setattr(K, attr, getattr(mod, attr))
    mods["config"].set_sample_rate(SR)
    doc, arrays = {"sr": SR, "facts": facts(K)}, {}
    all_cases = cases()
    for case in all_cases:
        case["same_as_whole"] = {}
        for pattern, blocks in case["patterns"].items():
            made = []
            pe = R.build(K, case["graph"], made)
            outs = H.render_blocks(pe, SR, blocks, case.get("ops"), lambda: H.reset_all(made),
                                   renderer=mods["null_renderer"].NullRenderer(sample_rate=SR),
                                   render=lambda s, n: np.ascontiguousarray(pe.render(s, n).data, dtype=np.float32))
            flat = np.concatenate(outs)
            assert flat.dtype == np.float32 and np.all(np.isfinite(flat)), case["name"]
            whole = arrays.get(f"{case['name']}/whole")
            same = pattern != "whole" and whole is not None and H.bits_equal(flat, whole)
            case["same_as_whole"][pattern] = bool(same)
            if not same:
                arrays[f"{case['name']}/{pattern}"] = flat
            peak = float(np.max(np.abs(flat)))
            if case["compare"] == "float":
                assert peak > 0.05, f"{case['name']}/{pattern}: peak {peak}: a silent case has no bar"
            print(f"{case['name']}/{pattern}: {flat.shape} {case['compare']} peak {peak:.6g}"
                  f"{' (= whole)' if same else ''}", flush=True)
    doc["cases"] = all_cases
    write_fixture("random_select", doc, arrays)


if __name__ == "__main__":
    main()
