"""
What ReversePitchEchoPE costs per block: the settings of the reference's examples/15_reverse_pitch_echo.py
(block_seconds=0.12, pitch_ratio=0.75, feedback=0.6, alternate_direction=1.0) at 44 100 Hz over 8 s of stereo noise
(an ArrayPE), pulled in blocks of 1 024 frames, of 16 384 frames (the reference AudioRenderer's chunk) and in one call.

    python tools/reverse_echo_probe.py --out profiles/reverse_echo_probe.jsonl          on an MI355X: rows "device"
    python tools/reverse_echo_probe.py --reference --out profiles/reverse_echo_probe.jsonl
                                            where the reference package is: rows "reference_cpu", the reference's kernel
                                            function _reverse_pitch_echo_numba INTERPRETED (numba absent) on the host CPU
    python tools/reverse_echo_probe.py --report profiles/reverse_echo_probe.jsonl       writes the .md beside it

Rows: microseconds of wall time per block and Msamples/s (frames x channels), a host clock around the sequential renders
of one pass over the stream in a started NullRenderer; on the device the clock stops after a synchronise.  A warm-up
pass and three timed ones; the report gives medians.  Each render of the PE is three launches (plan, pitch, echo); the
source's block is a view of the resident array.  The device step runs in a child process under a time limit.
Measured values, no gate.
"""

from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
FRAMES = 8 * SR
CHANNELS = 2
SETTINGS = dict(block_seconds=0.12, pitch_ratio=0.75, feedback=0.6, alternate_direction=1.0)
PULLS = (1024, 16384, FRAMES)
REPEATS = 4                  # the first warms up
LIMIT = 300                  # seconds allowed for the device step


def noise():
    return (np.random.default_rng(15).standard_normal((FRAMES, CHANNELS)) * 0.25).astype(np.float32)


def one_pass(K, renderer_type, block, sync):
    pe = K.ReversePitchEchoPE(K.ArrayPE(noise()), **SETTINGS)
    r = renderer_type(sample_rate=SR)
    r.set_source(pe)
    r.start()
    blocks = FRAMES // block
    sync()
    t0 = time.perf_counter()
    for i in range(blocks):
        pe.render(i * block, block)
    sync()
    seconds = time.perf_counter() - t0
    r.stop()
    return blocks, seconds


def rows(path, K, renderer_type, sync, emit):
    for block in PULLS:
        for repeat in range(REPEATS):
            blocks, seconds = one_pass(K, renderer_type, block, sync)
            emit({"path": path, "block": block, "blocks": blocks, "repeat": repeat, "warm_up": repeat == 0,
                  "us_per_block": round(seconds / blocks * 1e6, 2),
                  "msamples_per_s": round(blocks * block * CHANNELS / seconds / 1e6, 3)})


def device_step():
    import pygmu2_amd as pg
    from pygmu2_amd import device
    pg.set_sample_rate(SR)
    rows("device", pg, pg.NullRenderer, device.synchronize, lambda row: print(json.dumps(row), flush=True))


def reference_rows(emit):
    import importlib
    from oracle import gen_golden
    mods = gen_golden.load_reference()
    mod = importlib.import_module("pygmu2.reverse_pitch_echo_pe")
    K = mods["K"]
    K.ReversePitchEchoPE = mod.ReversePitchEchoPE
    mods["config"].set_sample_rate(SR)
    rows("reference_cpu", K, mods["null_renderer"].NullRenderer, lambda: None, emit)


def report(jsonl):
    table = {}
    for line in open(jsonl):
        row = json.loads(line)
        if not row["warm_up"]:
            table.setdefault((row["block"], row["path"]), []).append(row)
    lines = ["# ReversePitchEchoPE on an MI355X: `tools/reverse_echo_probe.py`", "",
             f"Raw rows: `{os.path.basename(jsonl)}`.  The settings of the reference's `examples/15_reverse_pitch_echo.py`"
             " (0.12 s blocks, ratio 0.75, feedback 0.6, alternating) at 44 100 Hz over 8 s of stereo noise.  Wall time of"
             " one pass over the stream, host clock, the device synchronised at both ends; medians of three passes after"
             " a warm-up pass, (min – max) beside them.  Msamples/s counts frames x channels.  `reference, CPU` is the"
             " reference's kernel function `_reverse_pitch_echo_numba` **interpreted** (numba absent) on a host"
             " CPU: what the fixtures are rendered with, not what a user with numba would see.", "",
             "| block (frames) | device, µs per block | device, Msamples/s | reference on the CPU (interpreted), µs per block |"
             " reference, Msamples/s |", "|---|---|---|---|---|"]

    def cell(block, path, key, digits):
        got = [r[key] for r in table.get((block, path), [])]
        if not got:
            return "not measured"
        return f"{statistics.median(got):,.{digits}f} ({min(got):,.{digits}f} – {max(got):,.{digits}f})".replace(",", " ")

    for block in PULLS:
        lines.append(f"| {block} | {cell(block, 'device', 'us_per_block', 1)} | {cell(block, 'device', 'msamples_per_s', 2)} | "
                     f"{cell(block, 'reference_cpu', 'us_per_block', 0)} | {cell(block, 'reference_cpu', 'msamples_per_s', 3)} |")
    lines += ["", "Every render of the PE is three launches -- plan, pitch, echo -- so two of three are the plan and pitch"
                  " stages; the echo stage runs one workgroup per channel and is latency-bound by design.  The kernels"
                  " alone were not measured (no `rocprofv3` run was made for this table)."]
    out = os.path.splitext(jsonl)[0] + ".md"
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(out)


def main():
    if "--step" in sys.argv:
        device_step()
        return 0
    if "--report" in sys.argv:
        report(sys.argv[sys.argv.index("--report") + 1])
        return 0
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None

    def emit(row_or_line):
        line = row_or_line if isinstance(row_or_line, str) else json.dumps(row_or_line) + "\n"
        sys.stdout.write(line)
        sys.stdout.flush()
        if out:
            out.write(line)
            out.flush()

    if "--reference" in sys.argv:
        reference_rows(emit)
        return 0
    import threading
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step"], stdout=subprocess.PIPE, text=True)
    watchdog = threading.Timer(LIMIT, p.kill)
    watchdog.start()
    try:
        for line in p.stdout:
            emit(line)
        status = p.wait()
    finally:
        watchdog.cancel()
    if status != 0:
        print(f"the step ended with status {status} (time limit {LIMIT} s); stopping", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
