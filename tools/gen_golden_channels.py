#!/usr/bin/env python3
"""
tools/gen_golden_channels.py -- TEST INFRASTRUCTURE ONLY; runs ONLY where the read-only reference tree exists (see
oracle/gen_golden.py, whose loader and builder it uses, and oracle/gen_golden_fuzz.py, which it is modelled on).

Renders every case of tests/channel_cases.py -- each channel-aware PE at 3, 4, 5 and 8 channels -- through the
reference's own classes and writes

    tests/golden/channels_cases.json    (case list: graph SPECs, blocks, stored block indices, sample rate, PE kind, C)
    tests/golden/channels.npz           (float32 outputs, key "<case>/<block index>")

Every block is rendered; each case stores the blocks of its `keep` list, chosen from the last block backwards within a
per-case sample budget.  The blocks that are not stored are checked against the oracle on the GPU
(tests/test_gpu_channels.py), and the oracle against the stored ones on the CPU (tests/test_oracle_channels.py).  The
archive is written with fixed member timestamps, so a re-run reproduces it bit for bit.

Usage:  PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_channels.py
"""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_golden import load_reference, render_case  # noqa: E402
from oracle.gen_golden_fuzz import choose_keep, write_npz                    # noqa: E402

BUDGET = 800          # stored samples (frames x channels) per case (a case may ask for its own), at least one block
CASES_PATH = os.path.join(ROOT, "tests", "golden", "channels_cases.json")
NPZ_PATH = os.path.join(ROOT, "tests", "golden", "channels.npz")


def main():
    import channel_cases
    import fuzz_graphs_all as F
    M = load_reference()
    arrays, stored = {}, []
    for case in channel_cases.cases():
        assert F.osc_edge_distance(case) > 1e-9, (case["name"], "a stateful oscillator on a waveform edge: redraw")
        outs = render_case(case, M)
        case["keep"] = choose_keep(outs, case.get("budget", BUDGET))
        for i in case["keep"]:
            arrays[f"{case['name']}/{i}"] = outs[i]
        stored.append(case)
        print(f"{case['name']:44s} blocks={len(case['blocks'])} keep={case['keep']} shape={outs[-1].shape}", flush=True)
    os.makedirs(os.path.dirname(NPZ_PATH), exist_ok=True)
    write_npz(NPZ_PATH, arrays)
    with open(CASES_PATH, "w") as f:
        json.dump(stored, f, separators=(",", ":"))
        f.write("\n")
    total = os.path.getsize(NPZ_PATH) + os.path.getsize(CASES_PATH)
    print(f"{len(stored)} cases, {len(arrays)} blocks, channels.npz + channels_cases.json = {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
