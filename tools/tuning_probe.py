"""
What a pitch stream turned into a frequency stream costs: the graph of the reference's examples/33_piecewise.py
(PiecewisePE -> TransformPE(pitch_to_freq) -> FunctionGenPE sawtooth -> GainPE, 8 s at 44.1 kHz), rendered in blocks of
512 frames and in one render, with the transform given as
  function   func=pitch_to_freq itself: lowered to pgx_tuning where the package lowers it, else the host callable;
  lambda     the same thing wrapped in a lambda: always the host callable (device -> host -> numpy -> device);
  explicit   transforms.PitchToFreq(EqualTemperament(12), 69.0, 440.0): nothing follows the globals, so read-ahead
             and look-ahead windows open (only where the package has the descriptor).
The first two exist on every commit, so the same file measures the commit before the tuning kernel too: run it from
either tree and put the rows side by side.  Rows: milliseconds of wall time per rendered second (host clock around the
renders, the device synchronised at both ends), three repeats, the variants alternating within a repeat.
  kernel     pgx_tuning alone, equal and just (12 notes), 512 and 352 800 frames per launch: microseconds per launch by
             HIP events on the library stream around at least 0.25 s of repeated launches after warm-up.

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  One JSON line per
row and repeat on stdout (and in --out FILE).  Measured values, no gate.
    python tools/tuning_probe.py [--out profiles/tuning_probe.jsonl] [--label NAME]
One step alone:
    python tools/tuning_probe.py --step stream|kernel
"""

from __future__ import annotations

import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
SECONDS = 8
BLOCK = 512
STEPS = {"stream": 240, "kernel": 120}           # seconds allowed per step
MIN_SECONDS = 0.25
LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else ""


def emit(**row):
    if LABEL:
        row["label"] = LABEL
    print(json.dumps(row), flush=True)


def triad(pg, func):
    pts = [(int(SR * t), p) for t, p in ((0, 60), (1.5, 60), (2, 64), (3.5, 64), (4, 67), (5.5, 67), (6, 60), (7.5, 60))]
    pitch = pg.PiecewisePE(pts, transition_type=pg.TransitionType.LINEAR, extend_mode=pg.ExtendMode.HOLD_LAST)
    freq = pg.TransformPE(pitch, func=func, name="pitch_to_freq")
    return pg.GainPE(pg.FunctionGenPE(frequency=freq, duty_cycle=0.5, waveform="sawtooth"), 0.25), freq


def step_stream():
    import pygmu2_amd as pg
    from pygmu2_amd import device, transforms
    pg.set_sample_rate(SR)
    variants = {"function": lambda: pg.pitch_to_freq, "lambda": lambda: (lambda v: pg.pitch_to_freq(v))}
    if hasattr(transforms, "PitchToFreq"):
        variants["explicit"] = lambda: transforms.PitchToFreq(pg.EqualTemperament(12), 69.0, 440.0)
    total = SR * SECONDS
    shapes = {"blocks_512": [(s, min(BLOCK, total - s)) for s in range(0, total, BLOCK)], "one_render": [(0, total)]}
    for repeat in range(4):                      # repeat 0 warms up (first launches, pool growth) and is marked
        for shape, requests in shapes.items():
            for name, make in variants.items():
                pe, freq = triad(pg, make())
                r = pg.NullRenderer(sample_rate=SR)
                r.set_source(pe)
                r.start()
                device.synchronize()
                t0 = time.perf_counter()
                for s, n in requests:
                    pe.render(s, n)
                device.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                r.stop()
                emit(row="stream", variant=name, shape=shape, repeat=repeat, warm_up=repeat == 0,
                     lowered=getattr(freq, "_lowered", None) is not None, renders=len(requests),
                     ms_per_rendered_second=round(ms / SECONDS, 4))


def time_launches(device, launch):
    for _ in range(10):
        launch()
    device.synchronize()
    t0, t1 = device.Event(), device.Event()
    t0.record()
    for _ in range(20):
        launch()
    t1.record()
    per = max(t1.elapsed_ms_since(t0) / 20, 1e-4)
    steps = int(min(200_000, max(20, math.ceil(MIN_SECONDS * 1e3 / per))))
    t0.record()
    for _ in range(steps):
        launch()
    t1.record()
    return t1.elapsed_ms_since(t0) * 1e3 / steps, steps


def step_kernel():
    import pygmu2_amd as pg
    from pygmu2_amd import device
    lib = device.ensure_init()
    if not hasattr(lib, "pgx_tuning"):
        emit(row="kernel", note="this build has no pgx_tuning")
        return
    from pygmu2_amd import transforms
    pg.set_sample_rate(SR)
    for n in (BLOCK, SR * SECONDS):
        x = device.DeviceBuffer.from_host(np.random.default_rng(1).uniform(36.0, 96.0, (n, 1)).astype(np.float32))
        out = device.DeviceBuffer((n, 1), np.float32)
        plain = np.zeros(1, dtype=device.TRANSFORM_OP)
        plain[0] = (0, 0, 2.0, 1.0)
        plain_dev = device.DeviceBuffer.from_host(plain.view(np.uint8))
        sides = {"k_transform affine": lambda: device.check(lib.pgx_transform(out.ptr, x.ptr, n, plain_dev.ptr, 1))}
        keep = []
        for name, temp in (("equal 12", pg.EqualTemperament(12)), ("just 12", pg.JustIntonation())):
            (code, tuning, _), = transforms.PitchToFreq(temp, 69.0, 440.0).ops()
            ops = np.zeros(1, dtype=device.TUNING_OP)
            ops[0] = (code, 0, 0.0, 0.0)
            rec = np.zeros(1, dtype=device.TUNING_RECORD)
            rec[0] = (tuning.reference_pitch, tuning.reference_freq, tuning.divisions, 0,
                      (len(tuning.table) - 1) // 2 if tuning.just else 0, 0)
            bufs = (device.DeviceBuffer.from_host(ops.view(np.uint8)), device.DeviceBuffer.from_host(rec.view(np.uint8)),
                    device.DeviceBuffer.from_host(np.asarray(tuning.table if tuning.just else np.zeros(1))))
            keep.append(bufs)
            sides[f"k_tuning {name}"] = (lambda b=bufs: device.check(
                lib.pgx_tuning(out.ptr, x.ptr, n, b[0].ptr, 1, b[1].ptr, b[2].ptr)))
        for repeat in range(3):
            for name, launch in sides.items():
                us, steps = time_launches(device, launch)
                emit(row="kernel", kernel=name, frames=n, repeat=repeat, launches=steps, us_per_launch=round(us, 3),
                     gb_per_s=round(8.0 * n / us * 1e-3, 2))


def main():
    if "--step" in sys.argv:
        {"stream": step_stream, "kernel": step_kernel}[sys.argv[sys.argv.index("--step") + 1]]()
        return 0
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None
    extra = ["--label", LABEL] if LABEL else []
    for step, limit in STEPS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + extra, capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if out:
            out.write(p.stdout)
            out.flush()
        if p.returncode != 0:
            print(f"step {step}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
