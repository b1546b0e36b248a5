"""
What TralfamPE costs on the device, per length (16 964, 132 300 x 2, 156 168 x 2, 2^20, 2^21 - 1), in one run:
  first      the first render of a fresh TralfamPE over a resident ArrayPE, end to end on the host clock, device wait
             included: the pull of the source, the plan of the length if it is new, workspace, pgx_tralfam, synchronise.
             Two rows per length: with a new length (plan made) and again with the plan resident;
  pipeline   pgx_tralfam alone -- load, DFT, phases, inverse DFT, store (+ peak and scale) -- by HIP events on the
             library stream around repeated calls after warm-up, three repeats; with the bytes the transforms move
             computed from the shapes (per FFT_M: passes x 32 B x M; Bluestein runs two FFT_M per transform, a power of
             two one) and that traffic's share of 8 TB/s of HBM bandwidth;
  dft        pgx_dft_c2c forward alone, batch 1, the same way;
  reference  the reference's TralfamPE on the CPU of the host this runs on, the same shapes (needs the reference
             package, oracle.gen_golden.load_reference; no device is touched).  Not part of the default run.

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  One JSON line per
row and repeat on stdout (and in --out FILE).  Measured values, no gate.
    python tools/tralfam_probe.py [--out profiles/tralfam_probe.jsonl]
One step alone:
    python tools/tralfam_probe.py --step first|pipeline|dft|reference|once
`--step once` renders each shape once through TralfamPE and nothing else, for a profiler run of its own
(`rocprofv3 --kernel-trace --stats -- python tools/tralfam_probe.py --step once`).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 48000
SHAPES = ((16_964, 1), (132_300, 2), (156_168, 2), (2 ** 20, 1), (2 ** 21 - 1, 1))
STEPS = {"first": 240, "pipeline": 240, "dft": 240}           # seconds allowed per step
MIN_SECONDS = 0.25
HBM_BYTES_PER_S = 8.0e12


def emit(**row):
    print(json.dumps(row), flush=True)


def fft_points(n):
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def fft_bytes(n, batch):
    """HBM bytes the power-of-two transforms of ONE DFT of `batch` sequences move: passes x 32 B x M each."""
    m = fft_points(n)
    passes = 1 if m <= 2048 else 2
    ffts = 1 if m == n else 2
    return ffts * passes * 32 * m * batch


def signal(n, channels):
    import tralfam_oracle as T
    return T.make_signal({"kind": "noise_decay", "n": n, "channels": channels}, None)


def time_calls(device, call):
    for _ in range(3):
        call()
    device.synchronize()
    t0, t1 = device.Event(), device.Event()
    t0.record()
    for _ in range(3):
        call()
    t1.record()
    per = max(t1.elapsed_ms_since(t0) / 3, 1e-4)
    steps = int(min(20_000, max(3, math.ceil(MIN_SECONDS * 1e3 / per))))
    t0.record()
    for _ in range(steps):
        call()
    t1.record()
    return t1.elapsed_ms_since(t0) * 1e3 / steps, steps


def step_first():
    import pygmu2_amd as pg
    from pygmu2_amd import device, spectral
    pg.set_sample_rate(SR)
    pg.ArrayPE(np.zeros(8, dtype=np.float32)).render(0, 8).dev       # library up, pools warm
    device.synchronize()
    for n, ch in SHAPES:
        src = pg.ArrayPE(signal(n, ch))
        src.render(0, n).dev
        device.synchronize()
        spectral.plan_for.cache_clear()
        for repeat, plan in enumerate(("new", "resident", "resident")):
            pe = pg.TralfamPE(src, seed=1, normalize_peak=0.5)
            t = time.perf_counter()
            pe.render(0, n)
            device.synchronize()
            dt = time.perf_counter() - t
            emit(row="first", frames=n, channels=ch, plan=plan, repeat=repeat, us=round(dt * 1e6, 1))


def step_pipeline():
    from pygmu2_amd import device, spectral
    lib = device.ensure_init()
    for n, ch in SHAPES:
        x = device.DeviceBuffer.from_host(signal(n, ch))
        out = device.DeviceBuffer((n, ch), np.float32)
        plan = spectral.plan_for(n)
        work = device.DeviceBuffer((lib.pgx_tralfam_workspace_bytes(n, ch),), np.uint8)
        s = np.random.PCG64(1).state["state"]
        rec = np.zeros(1, dtype=device.NOISE_PARAMS)
        rec["state_hi"], rec["state_lo"] = int(s["state"]) >> 64, int(s["state"]) & (2 ** 64 - 1)
        rec["inc_hi"], rec["inc_lo"] = int(s["inc"]) >> 64, int(s["inc"]) & (2 ** 64 - 1)
        rng = device.upload_structs(rec)
        moved = 2 * fft_bytes(n, ch)                              # a forward and an inverse DFT
        for normalize in (0.0, 0.5):
            def call():
                device.check(lib.pgx_tralfam(out.ptr, x.ptr, n, ch, rng.ptr, normalize, plan.buf.ptr, work.ptr),
                             "pgx_tralfam")
            for repeat in range(3):
                us, steps = time_calls(device, call)
                emit(row="pipeline", frames=n, channels=ch, fft_points=fft_points(n), normalize=bool(normalize),
                     repeat=repeat, calls=steps, us_per_call=round(us, 2), fft_bytes=moved,
                     fft_gb_per_s=round(moved / us * 1e-3, 1),
                     hbm_share=round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 4))


def step_dft():
    from pygmu2_amd import device, spectral
    lib = device.ensure_init()
    for n, _ in SHAPES + ((2 ** 21, 1), (4096, 1), (2048, 1)):
        rng = np.random.default_rng(n)
        x = device.DeviceBuffer.from_host((rng.standard_normal((n, 2))))
        out = device.DeviceBuffer((n, 2), np.float64)
        plan = spectral.plan_for(n)
        work = device.DeviceBuffer((lib.pgx_dft_workspace_bytes(n, 1),), np.uint8)

        def call():
            device.check(lib.pgx_dft_c2c(out.ptr, x.ptr, n, 1, 0, plan.buf.ptr, work.ptr), "pgx_dft_c2c")
        moved = fft_bytes(n, 1)
        for repeat in range(3):
            us, steps = time_calls(device, call)
            emit(row="dft", frames=n, fft_points=fft_points(n), repeat=repeat, calls=steps, us_per_call=round(us, 2),
                 fft_bytes=moved, fft_gb_per_s=round(moved / us * 1e-3, 1),
                 hbm_share=round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 4))


def step_once():
    import pygmu2_amd as pg
    from pygmu2_amd import device
    pg.set_sample_rate(SR)
    for n, ch in SHAPES:
        pe = pg.TralfamPE(pg.ArrayPE(signal(n, ch)), seed=1, normalize_peak=0.5)
        pe.render(0, n)
        device.synchronize()
        emit(row="once", frames=n, channels=ch, renders=1)


def step_reference():
    import importlib
    from oracle import gen_golden
    mods = gen_golden.load_reference()
    tralfam_pe = importlib.import_module("pygmu2.tralfam_pe")
    mods["config"].set_sample_rate(SR)
    for n, ch in SHAPES:
        src = mods["array_pe"].ArrayPE(signal(n, ch))
        for repeat in range(3):
            renders, t = 0, time.perf_counter()
            while time.perf_counter() - t < MIN_SECONDS or renders < 1:
                tralfam_pe.TralfamPE(src, seed=1, normalize_peak=0.5).render(0, n)
                renders += 1
            dt = time.perf_counter() - t
            emit(row="reference_cpu", frames=n, channels=ch, repeat=repeat, renders=renders,
                 us_per_first_render=round(dt * 1e6 / renders, 1), numpy=np.__version__)


def main():
    args = sys.argv[1:]
    if "--step" in args:
        {"first": step_first, "pipeline": step_pipeline, "dft": step_dft, "once": step_once,
         "reference": step_reference}[args[args.index("--step") + 1]]()
        return 0
    out = args[args.index("--out") + 1] if "--out" in args else None
    lines = []
    for step, limit in STEPS.items():
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True,
                              text=True, timeout=limit)
        sys.stdout.write(proc.stdout)
        sys.stdout.flush()
        lines += [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            print(f"step {step} failed with status {proc.returncode}: stopping", file=sys.stderr)
            return 1
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
