"""
What the control-signal kernels cost, each beside a comparator that exists without them, in the same run:
  hold      pgx_hold (mono source, mono control, a pass every 128 frames) beside pgx_gain_vec on mono streams of the
            same length -- identical traffic: two float32 streams in, one out;
  slew      pgx_slew, LINEAR and EXPONENTIAL with rise >> fall, beside pgx_envelope with attack != release (the same
            coefficients, the same input) for a staircase, noise and a slow sine; the Newton round counts of each
            (inner rounds per 8192-frame window, window-level rounds) from the kernel's own counters;
  fgen      pgx_function_gen_stateful (sawtooth and rectangle) beside pgx_gate_stateful, both with a frequency stream;
  stream    the four PEs pulled in 1024-frame blocks through look-ahead windows (frames per second, whole graph).
Kernel rows: 48 000 and 2^20 frames per launch, HIP events on the library stream around at least 0.25 s of repeated
launches after warm-up, three repeats with the two sides alternating.

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  One JSON line per
row and repeat on stdout (and in --out FILE).  Measured values, no gate.
    python tools/control_probe.py [--out profiles/control_probe.jsonl]
One step alone, for a profiler run of its own (kernel times by `rocprofv3 --kernel-trace --stats -- python ...`):
    python tools/control_probe.py --step hold|slew|fgen|stream [--frames N]
"""

from __future__ import annotations

import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 48000
SIZES = (48_000, 1 << 20)
STEPS = {"hold": 120, "slew": 240, "fgen": 120, "stream": 240}           # seconds allowed per step
MIN_SECONDS = 0.25


def emit(**row):
    print(json.dumps(row), flush=True)


def time_launches(device, launch):
    """microseconds per launch: warm-up, then events around >= MIN_SECONDS of launches."""
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


def sources(n):
    rng = np.random.default_rng(3)
    noise = (0.5 * rng.standard_normal(n)).astype(np.float32)
    stair = np.repeat(noise[::128], 128)[:n]
    sine = (0.5 * np.sin(2 * np.pi * 20.0 * np.arange(n) / SR)).astype(np.float32)
    return {"staircase": stair, "noise": noise, "sine": sine}


def step_hold():
    from pygmu2_amd import device
    lib = device.ensure_init()
    for n in SIZES:
        rng = np.random.default_rng(1)
        src = device.DeviceBuffer.from_host(rng.standard_normal((n, 1)).astype(np.float32))
        ctl_host = np.zeros((n, 1), np.float32)
        ctl_host[::128] = 1.0
        ctl = device.DeviceBuffer.from_host(ctl_host)
        out = device.DeviceBuffer((n, 1), np.float32)
        state = device.DeviceBuffer((1,), np.float64, zero=True)
        work = device.DeviceBuffer((1040,), np.float64)
        sides = {
            "pgx_hold": lambda: device.check(lib.pgx_hold(out.ptr, src.ptr, 1, ctl.ptr, 1, n, 0.0, state.ptr, work.ptr), "pgx_hold"),
            "pgx_gain_vec": lambda: device.check(lib.pgx_gain_vec(out.ptr, src.ptr, ctl.ptr, n, 1, 1), "pgx_gain_vec"),
        }
        for repeat in range(3):
            for name, launch in sides.items():
                us, steps = time_launches(device, launch)
                emit(row="hold", kernel=name, frames=n, repeat=repeat, launches=steps, us_per_launch=round(us, 3),
                     gb_per_s=round(12.0 * n / us * 1e-3, 1))


def step_slew():
    from pygmu2_amd import device
    lib = device.ensure_init()
    up, down = 2000.0 / SR, 5.0 / SR
    for n in SIZES:
        out = device.DeviceBuffer((n, 1), np.float32)
        state = device.DeviceBuffer((1,), np.float64, zero=True)
        scratch = device.DeviceBuffer((max(1, lib.pgx_slew_scratch_bytes(n) // 8),), np.float64)
        env_scratch = device.DeviceBuffer((lib.pgx_envelope_scratch_bytes(n, 1) // 8,), np.float64)
        stats = device.DeviceBuffer((4,), np.int32, zero=True)
        for sname, host in sources(n).items():
            x = device.DeviceBuffer.from_host(host.reshape(-1, 1))

            def slew(mode, counters=None):
                device.check(lib.pgx_slew(out.ptr, x.ptr, 1, n, mode, up, down, state.ptr, scratch.ptr,
                                          None if counters is None else counters.ptr), "pgx_slew")
            sides = {
                "pgx_slew_linear": lambda: slew(0),
                "pgx_slew_exponential": lambda: slew(1),
                "pgx_envelope": lambda: device.check(lib.pgx_envelope(out.ptr, x.ptr, n, 1, up, down, 0, 0, 0, state.ptr,
                                                                      env_scratch.ptr), "pgx_envelope"),
            }
            for mode, name in ((0, "pgx_slew_linear"), (1, "pgx_slew_exponential")):
                state.zero_()
                stats.zero_()
                slew(mode, stats)
                inner, windows, outer, fallbacks = (int(v) for v in stats.to_host())
                emit(row="slew_rounds", kernel=name, source=sname, frames=n, inner_rounds=inner, window_solves=windows,
                     inner_rounds_per_solve=round(inner / max(windows, 1), 2), window_level_rounds=outer,
                     fallbacks=fallbacks)
            for repeat in range(3):
                for name, launch in sides.items():
                    state.zero_()
                    us, steps = time_launches(device, launch)
                    emit(row="slew", kernel=name, source=sname, frames=n, repeat=repeat, launches=steps,
                         us_per_launch=round(us, 3), mframes_per_s=round(n / us, 1))


def step_fgen():
    from pygmu2_amd import device
    lib = device.ensure_init()
    for n in SIZES:
        freq_host = (440.0 + 20.0 * np.sin(2 * np.pi * 5.0 * np.arange(n) / SR)).astype(np.float32)
        freq = device.DeviceBuffer.from_host(freq_host.reshape(-1, 1))
        out = device.DeviceBuffer((n, 1), np.float32)
        state = device.DeviceBuffer((1,), np.float64, zero=True)
        work = device.DeviceBuffer((1040,), np.float64)

        def fgen(saw):
            device.check(lib.pgx_function_gen_stateful(out.ptr, n, 1, saw, float(SR), 0.0, 0.3, 0.0, freq.ptr, None, None,
                                                       state.ptr, work.ptr), "pgx_function_gen_stateful")
        sides = {
            "pgx_function_gen_stateful_rectangle": lambda: fgen(0),
            "pgx_function_gen_stateful_sawtooth": lambda: fgen(1),
            "pgx_gate_stateful": lambda: device.check(lib.pgx_gate_stateful(out.ptr, n, float(SR), 0.0, 0.3, 0.0, freq.ptr,
                                                                            None, None, state.ptr), "pgx_gate_stateful"),
        }
        for repeat in range(3):
            for name, launch in sides.items():
                us, steps = time_launches(device, launch)
                emit(row="fgen", kernel=name, frames=n, repeat=repeat, launches=steps, us_per_launch=round(us, 3),
                     mframes_per_s=round(n / us, 1))


def step_stream():
    import pygmu2_amd as pg
    from pygmu2_amd import device, look_ahead
    pg.set_sample_rate(SR)
    noise = (0.5 * np.random.default_rng(9).standard_normal(1 << 22)).astype(np.float32)
    vib = lambda: pg.TransformPE(pg.SinePE(5.0), func=pg.transforms.Affine(20.0, 440.0))      # noqa: E731
    stair = lambda: pg.SampleHoldPE(pg.ArrayPE(noise), pg.PeriodicTrigger(375.0))              # noqa: E731
    graphs = {
        "SampleHoldPE(noise, PeriodicTrigger)": stair,
        "TrackHoldPE(noise, PeriodicGate)": lambda: pg.TrackHoldPE(pg.ArrayPE(noise), pg.PeriodicGate(200.0, 0.3)),
        "SlewLimiterPE(SampleHoldPE) linear": lambda: pg.SlewLimiterPE(stair(), 2000.0, 5.0),
        "SlewLimiterPE(SampleHoldPE) exponential": lambda: pg.SlewLimiterPE(stair(), 2000.0, 5.0, pg.SlewMode.EXPONENTIAL),
        "FunctionGenPE(vibrato) sawtooth": lambda: pg.FunctionGenPE(vib(), 0.3, 0.0, "sawtooth"),
        "PeriodicGate(vibrato)": lambda: pg.PeriodicGate(vib(), 0.3),
    }
    blocks, block = 3000, 1024
    for name, make in graphs.items():
        for repeat in range(3):
            for ahead in (True, False):
                look_ahead.set_enabled(ahead)
                pe = make()
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
                emit(row="stream", graph=name, block=block, blocks=blocks, look_ahead=ahead, repeat=repeat,
                     us_per_block=round(ms * 1e3 / blocks, 3), mframes_per_s=round(blocks * block / ms * 1e-3, 1))
    look_ahead.set_enabled(True)


def main():
    if "--step" in sys.argv:
        if "--frames" in sys.argv:
            global SIZES
            SIZES = (int(sys.argv[sys.argv.index("--frames") + 1]),)
        {"hold": step_hold, "slew": step_slew, "fgen": step_fgen, "stream": step_stream}[sys.argv[sys.argv.index("--step") + 1]]()
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
