"""
What the NoisePE kernels cost, in one run:
  kernels    pgx_noise_white / _pink / _brown, one instance, 1024, 48 000 and 1 000 000 frames per launch, WHITE beside
             pgx_fill on a buffer of the same length (the same 4 B per frame written and nothing computed); WHITE's
             achieved write bandwidth against those 4 B per frame;
  bank       the same entry points with 256 instances of 48 000 frames in one launch (what fills the machine when one
             PINK / BROWN instance cannot: its recurrence is stepped literally);
  pe         NoisePE.render through the public class, 1 000 000 frames per render, look-ahead off, host clock around
             renders that each end in a device synchronise;
  stream     NoisePE pulled in 1024-frame blocks, look-ahead windows on and off;
  reference  the reference's NoisePE on the CPU of the host this runs on, the same three lengths (needs the reference
             package, oracle.gen_golden.load_reference; no device is touched).  Not part of the default run.
Kernel rows: HIP events on the library stream around at least 0.25 s of repeated launches after warm-up, three repeats
with the sides alternating.

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  One JSON line per
row and repeat on stdout (and in --out FILE).  Measured values, no gate.
    python tools/noise_probe.py [--out profiles/noise_probe.jsonl]
One step alone:
    python tools/noise_probe.py --step kernels|bank|pe|stream|reference|once
`--step once` renders 1 000 000 frames of each mode once through NoisePE and nothing else, for a profiler run of its
own (`rocprofv3 --kernel-trace --stats -- python tools/noise_probe.py --step once`: one k_noise_* dispatch per render).
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

SR = 48000
SIZES = (1024, 48_000, 1_000_000)
STEPS = {"kernels": 240, "bank": 120, "pe": 120, "stream": 240}           # seconds allowed per step
MIN_SECONDS = 0.25
MODES = ("white", "pink", "brown")


def emit(**row):
    print(json.dumps(row), flush=True)


def time_launches(device, launch):
    """microseconds per launch: warm-up, then events around >= MIN_SECONDS of launches."""
    for _ in range(5):
        launch()
    device.synchronize()
    t0, t1 = device.Event(), device.Event()
    t0.record()
    for _ in range(5):
        launch()
    t1.record()
    per = max(t1.elapsed_ms_since(t0) / 5, 1e-4)
    steps = int(min(200_000, max(5, math.ceil(MIN_SECONDS * 1e3 / per))))
    t0.record()
    for _ in range(steps):
        launch()
    t1.record()
    return t1.elapsed_ms_since(t0) * 1e3 / steps, steps


def noise_params(device, batch):
    rec = np.zeros(batch, dtype=device.NOISE_PARAMS)
    for i in range(batch):
        s = np.random.PCG64(1000 + i).state["state"]
        state, inc = int(s["state"]), int(s["inc"])
        rec[i]["state_hi"], rec[i]["state_lo"] = state >> 64, state & (2 ** 64 - 1)
        rec[i]["inc_hi"], rec[i]["inc_lo"] = inc >> 64, inc & (2 ** 64 - 1)
    return device.upload_structs(rec)


def launches(device, lib, batch, n):
    out = device.DeviceBuffer((batch, n), np.float32)
    params = noise_params(device, batch)
    state = device.DeviceBuffer((batch,), device.NOISE_STATE, zero=True)
    keep = (out, params, state)
    return keep, {
        "pgx_noise_white": lambda: device.check(lib.pgx_noise_white(out.ptr, n, batch, n, 12345, params.ptr), "white"),
        "pgx_noise_pink": lambda: device.check(lib.pgx_noise_pink(out.ptr, n, batch, n, 12345, params.ptr, state.ptr), "pink"),
        "pgx_noise_brown": lambda: device.check(lib.pgx_noise_brown(out.ptr, n, batch, n, 12345, params.ptr, state.ptr), "brown"),
        "pgx_fill": lambda: device.check(lib.pgx_fill(out.ptr, batch * n, 0.5), "pgx_fill"),
    }


def step_kernels(batch=1, sizes=SIZES, row="kernels"):
    from pygmu2_amd import device
    lib = device.ensure_init()
    for n in sizes:
        keep, sides = launches(device, lib, batch, n)
        for repeat in range(3):
            for name, launch in sides.items():
                us, steps = time_launches(device, launch)
                emit(row=row, kernel=name, instances=batch, frames=n, repeat=repeat, launches=steps,
                     us_per_launch=round(us, 3), mframes_per_s=round(batch * n / us, 2),
                     write_gb_per_s=round(4.0 * batch * n / us * 1e-3, 2))
        del keep


def step_bank():
    step_kernels(batch=256, sizes=(48_000,), row="bank")


def step_pe():
    import pygmu2_amd as pg
    from pygmu2_amd import device, look_ahead
    pg.set_sample_rate(SR)
    n = SIZES[-1]
    look_ahead.set_enabled(False)          # sequential pulls of this size would be served from windows: time renders
    for repeat in range(3):
        for mode in pg.NoiseMode:
            pe = pg.NoisePE(seed=1, mode=mode)
            r = pg.NullRenderer(sample_rate=SR)
            r.set_source(pe)
            r.start()
            for i in range(3):
                pe.render(i * n, n)
            device.synchronize()
            renders, t = 0, time.perf_counter()
            while time.perf_counter() - t < MIN_SECONDS or renders < 3:
                pe.render((3 + renders) * n, n)
                device.synchronize()
                renders += 1
            dt = time.perf_counter() - t
            r.stop()
            emit(row="pe", mode=mode.value, frames=n, repeat=repeat, renders=renders,
                 us_per_render=round(dt * 1e6 / renders, 1), mframes_per_s=round(renders * n / dt * 1e-6, 2))


def step_stream():
    import pygmu2_amd as pg
    from pygmu2_amd import device, look_ahead
    pg.set_sample_rate(SR)
    blocks, block = 2000, 1024
    for mode in pg.NoiseMode:
        for repeat in range(3):
            for ahead in (True, False):
                look_ahead.set_enabled(ahead)
                pe = pg.NoisePE(seed=1, mode=mode)
                r = pg.NullRenderer(sample_rate=SR)
                r.set_source(pe)
                r.start()
                for i in range(300):
                    pe.render(i * block, block)
                device.synchronize()
                t0, t1 = device.Event(), device.Event()
                t0.record()
                for i in range(300, 300 + blocks):
                    pe.render(i * block, block)
                t1.record()
                ms = t1.elapsed_ms_since(t0)
                r.stop()
                emit(row="stream", mode=mode.value, block=block, blocks=blocks, look_ahead=ahead, repeat=repeat,
                     us_per_block=round(ms * 1e3 / blocks, 3), mframes_per_s=round(blocks * block / ms * 1e-3, 2))
    look_ahead.set_enabled(True)


def step_once():
    import pygmu2_amd as pg
    from pygmu2_amd import device
    pg.set_sample_rate(SR)
    for mode in pg.NoiseMode:
        pe = pg.NoisePE(seed=1, mode=mode)
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(pe)
        r.start()
        pe.render(0, SIZES[-1])
        device.synchronize()
        r.stop()
        emit(row="once", mode=mode.value, frames=SIZES[-1], renders=1)


def step_reference():
    import importlib
    from oracle import gen_golden
    mods = gen_golden.load_reference()
    noise_pe = importlib.import_module("pygmu2.noise_pe")
    mods["config"].set_sample_rate(SR)
    for n in SIZES:
        for mode in noise_pe.NoiseMode:
            for repeat in range(3):
                pe = noise_pe.NoisePE(seed=1, mode=mode)
                r = mods["null_renderer"].NullRenderer(sample_rate=SR)
                r.set_source(pe)
                r.start()
                pe.render(0, min(n, 4096))
                renders, t = 0, time.perf_counter()
                while time.perf_counter() - t < MIN_SECONDS or renders < 1:
                    pe.render(renders * n, n)
                    renders += 1
                dt = time.perf_counter() - t
                r.stop()
                emit(row="reference_cpu", mode=mode.value, frames=n, repeat=repeat, renders=renders,
                     us_per_render=round(dt * 1e6 / renders, 1), mframes_per_s=round(renders * n / dt * 1e-6, 4),
                     numpy=np.__version__)


def main():
    table = {"kernels": step_kernels, "bank": step_bank, "pe": step_pe, "stream": step_stream, "once": step_once,
             "reference": step_reference}
    if "--step" in sys.argv:
        table[sys.argv[sys.argv.index("--step") + 1]]()
        return 0
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
    for step, limit in STEPS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True,
                               timeout=limit)
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
