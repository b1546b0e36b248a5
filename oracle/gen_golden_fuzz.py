#!/usr/bin/env python3
"""
oracle/gen_golden_fuzz.py -- TEST INFRASTRUCTURE ONLY; runs ONLY where the read-only reference tree exists (see
oracle/gen_golden.py, whose loader and builder it uses).

Renders a corpus of random graphs through the reference's own classes and writes

    tests/golden/fuzz_cases.json    (case list: graph SPECs, blocks, stored block indices, sample rate)
    tests/golden/fuzz.npz           (float32 outputs, key "<case>/<block index>")

The corpus: seeds 0..99 of tests/test_gpu_fuzz.py's `_graph`; short-block seeds of tests/fuzz_graphs_all.py plus a
few of its long and stream seeds; and hand-written cases for the interactions of the newest PEs with the processors
that re-address pulls.  Every block is rendered; each case stores the blocks of its `keep` list, chosen from the last
block backwards within a per-case sample budget (the state carried into a late block is what a kernel gets wrong).
The archive is written with fixed member timestamps, so a re-run reproduces it bit for bit.

Usage:  PYTHONDONTWRITEBYTECODE=1 python3 oracle/gen_golden_fuzz.py
"""

from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_golden import load_reference, render_case  # noqa: E402

N_OLD = 100           # seeds 0..99 of test_gpu_fuzz._graph
N_SHORT = 150         # short-block seeds of the new generator
N_LONG = 4            # long-block seeds (a 300-frame block appended: the one stored)
N_STREAM = 6          # stream seeds
BUDGET = 3584         # stored samples (frames x channels) per case, at least one block
CASES_PATH = os.path.join(ROOT, "tests", "golden", "fuzz_cases.json")
NPZ_PATH = os.path.join(ROOT, "tests", "golden", "fuzz.npz")


def _stream(start, n, count, back_at=None, back=0, seek_at=None, seek=0):
    blocks, pos = [], start
    for i in range(count):
        if i == back_at:
            pos -= back
        if i == seek_at:
            pos += seek
        blocks.append([pos, n])
        pos += n
    return blocks


def hand_cases():
    """The interactions that random draws reach only now and then, each spelled out once."""
    trig = {"pe": "PeriodicTrigger", "hz": 23.0}
    ks = {"pe": "KarplusStrongPE", "frequency": 196.0, "rho": 0.998, "duration": 2500, "rho_damping": 0.95,
          "amplitude": 0.5, "seed": 7, "channels": 1}
    ks_long = {"pe": "KarplusStrongPE", "frequency": 1.3, "rho": 1.0, "amplitude": 0.4, "seed": 11, "channels": 2}
    saw = {"pe": "AnalogOscPE", "frequency": 331.0, "duty_cycle": 0.3, "waveform": "sawtooth"}
    rect = {"pe": "AnalogOscPE", "frequency": 517.0, "duty_cycle": 0.41, "waveform": "rectangle"}
    sweep = {"pe": "PiecewisePE", "points": [[0, 90.0], [9000, 1370.0], [15000, -240.0]], "transition_type": "linear",
             "extend_mode": "hold_both"}
    saw_st = {"pe": "AnalogOscPE", "frequency": sweep,
              "duty_cycle": {"pe": "TransformPE", "source": {"pe": "SinePE", "frequency": 3.1},
                             "ops": [["affine", 0.35, 0.5]]}, "waveform": "sawtooth"}
    c_ks = dict({"pe": "CachePE", "source": ks}, share="c")
    c_bq = dict({"pe": "CachePE", "source": {"pe": "BiquadPE", "source": saw_st, "frequency": 1800.0, "q": 1.5,
                                            "mode": "lowpass"}}, share="c")
    s1024 = _stream(-300, 1024, 24, back_at=13, back=1500, seek_at=19, seek=3000)
    s256 = _stream(-100, 256, 40, back_at=25, back=300)
    cases = [
        ("hand_cache_mix_gain", {"pe": "MixPE", "inputs": [c_ks, {"pe": "GainPE", "source": c_ks, "gain": -0.5}]}, s1024),
        ("hand_cache_delay_beside", {"pe": "MixPE", "inputs": [{"pe": "DelayPE", "source": c_bq, "delay": 300}, c_bq]},
         s256),
        ("hand_cache_under_restart", {"pe": "TriggerRestartPE", "trigger": trig,
                                      "src": {"pe": "MixPE", "inputs": [c_ks, {"pe": "GainPE", "source": c_ks,
                                                                                "gain": 0.25}]}}, s1024),
        ("hand_ks_under_restart", {"pe": "TriggerRestartPE", "trigger": trig, "src": ks}, s1024),
        ("hand_window_over_ks", {"pe": "WindowPE", "source": ks, "window": 0.004, "mode": "max", "rectify": True}, s256),
        ("hand_saw_under_delay", {"pe": "DelayPE", "source": saw, "delay": 123}, s1024),
        ("hand_saw_under_loop", {"pe": "LoopPE", "source": {"pe": "CropPE", "source": saw, "start": 0, "duration": 5000,
                                                             "extend_mode": "zero"},
                                 "loop_start": 700, "loop_end": 2900, "count": None, "crossfade_seconds": 0.004},
         s256),
        ("hand_osc_mix_cropped", {"pe": "MixPE", "inputs": [
            {"pe": "CropPE", "source": rect, "start": 2000, "duration": 7000, "extend_mode": "zero"},
            {"pe": "CropPE", "source": saw_st, "start": -200, "duration": 12000, "extend_mode": "zero"}]}, s1024),
        ("hand_ks_delay_frac_stereo", {"pe": "DelayPE", "source": ks_long, "delay": 40.37, "interpolation": "cubic"},
         s1024),
        ("hand_ks_spatial_loop", {"pe": "SpatialPE", "source": {"pe": "LoopPE", "source": ks, "loop_start": 0,
                                                                 "loop_end": 3000, "count": 3},
                                  "method": "constant_power", "azimuth": 35.0}, s1024),
        ("hand_cache_same_start_other_length",
         {"pe": "MixPE", "inputs": [c_ks, {"pe": "GainPE", "source": c_ks, "gain": -0.75}]},
         [[0, 512], [512, 512], [512, 300], [812, 212], [1024, 1024], [1024, 64], [1088, 960], [2048, 1024]]),
        ("hand_identity_trigger_restart", {"pe": "TriggerRestartPE", "trigger": {"pe": "PeriodicTrigger", "hz": 7.0},
                                           "src": {"pe": "GainPE", "source": {"pe": "IdentityPE"}, "gain": 1e-4}},
         s1024),
    ]
    return [{"name": name, "sr": 44100, "graph": g, "blocks": b} for name, g, b in cases]


def corpus():
    import fuzz_graphs_all as F
    import test_gpu_fuzz
    out = []
    for seed in range(N_OLD):
        case = test_gpu_fuzz._graph(seed)
        out.append({"name": case["name"], "sr": case["sr"], "graph": case["graph"], "blocks": case["blocks"]})
    for pattern, count in (("short", N_SHORT), ("long", N_LONG), ("stream", N_STREAM)):
        for seed in range(count):
            case = F.make_case(pattern, seed)
            if pattern == "long":
                s, n = case["blocks"][-1]
                case["blocks"].append([s + n, 300])
            out.append({"name": case["name"], "sr": case["sr"], "graph": case["graph"], "blocks": case["blocks"]})
    hand = hand_cases()
    for case in hand:
        assert F.osc_edge_distance(case) > 1e-9, case["name"]
    return out + hand


def choose_keep(outs, budget=BUDGET):
    """Blocks from the last backwards while they fit the budget; the smallest block if none does."""
    keep, left = [], budget
    for i in range(len(outs) - 1, -1, -1):
        size = outs[i].size
        if size <= left:
            keep.append(i)
            left -= size
    if not keep:
        keep = [int(np.argmin([o.size for o in outs]))]
    return sorted(keep)


def write_npz(path, arrays):
    """np.savez_compressed's layout with fixed member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    M = load_reference()
    arrays, stored = {}, []
    for case in corpus():
        outs = render_case(case, M)
        case["keep"] = choose_keep(outs)
        for i in case["keep"]:
            arrays[f"{case['name']}/{i}"] = outs[i]
        stored.append(case)
        print(f"{case['name']:36s} blocks={len(case['blocks'])} keep={case['keep']}")
    os.makedirs(os.path.dirname(NPZ_PATH), exist_ok=True)
    write_npz(NPZ_PATH, arrays)
    with open(CASES_PATH, "w") as f:
        json.dump(stored, f, separators=(",", ":"))
        f.write("\n")
    total = os.path.getsize(NPZ_PATH) + os.path.getsize(CASES_PATH)
    print(f"{len(stored)} cases, {len(arrays)} blocks, fuzz.npz + fuzz_cases.json = {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
