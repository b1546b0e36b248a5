#!/usr/bin/env python3
"""pgx_biquad_sine at 16 M, 33 M, 2^26 and 134 M frames: the single-launch filter kernel (wave runs off) against the
wave-run kernel (k_biquad_sine_runs, forced on at any run length), alternated, HIP-event time per launch (GPU box).
The wave-run threshold (kRunMinChunks, pgx_biquad.hip) is set from these numbers."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import pygmu2_amd as pg
from pygmu2_amd import device

lib = device.ensure_init()
rows = []
for frames, launches in ((16_000_000, 100), (33_000_000, 50), (1 << 26, 30), (134_000_000, 20)):
    t = {"current": [], "runs": []}
    for rep in range(3):
        for name, min_chunks in (("current", 0), ("runs", 1)):
            lib.pgx_biquad_sine_set_runs(min_chunks)
            r = bench.biquad_sine_roofline(pg, frames, launches, 10 ** 9)
            t[name].append(r["avg_launch_ms"] * 1e3)
    lib.pgx_biquad_sine_set_runs(-1)
    row = {"frames": frames, "current_us": sorted(t["current"]), "runs_us": sorted(t["runs"]),
           "speedup": round(sorted(t["current"])[1] / sorted(t["runs"])[1], 3)}
    rows.append(row)
    print(json.dumps(row), flush=True)
