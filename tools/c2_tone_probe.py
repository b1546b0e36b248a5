#!/usr/bin/env python3
"""A BiquadPE(SinePE) window in closed form (pgx_biquad_tone, csrc/pgx_tone.hip) against the wave-run kernel
(pgx_biquad_sine -> k_biquad_sine_runs) at 16 M, 33 M, 2^26 and 134 M frames: the C2 chain, both entries called as a
look-ahead window calls them (carried state in, no snapshot), HIP events over streams of 20 - 40 ms of launches after
half as many untimed (tools/c2_window_phases.py's protocol), one process per variant, variants interleaved.

    python tools/c2_tone_probe.py run [--out DIR] [--passes N]     # GPU; writes DIR/c2_tone.jsonl and DIR/c2_tone.md

DIR defaults to runs/.  An existing c2_tone.md keeps everything below its line `<!-- probe table above -->`.
"""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16_000_000, 1000), (33_000_000, 600), (1 << 26, 400), (134_000_000, 300))
SR = 44100.0
VARIANTS = ("runs", "tone")
MARK = "<!-- probe table above -->"


def worker(variant):
    import numpy as np
    sys.path.insert(0, ROOT)
    import pygmu2_amd as pg
    from pygmu2_amd import device
    from pygmu2_amd.biquad_pe import rbj_coefficients, settle_frames
    lib = device.ensure_init()
    c = rbj_coefficients(pg.BiquadMode.LOWPASS, 1000.0, 0.707, 0.0, SR)
    coef = device.DeviceBuffer.from_host(np.asarray(c, dtype=np.float64))
    settle = settle_frames(c[3], c[4])
    tables = device.DeviceBuffer((lib.pgx_biquad_table_doubles(),), np.float64)
    device.check(lib.pgx_biquad_tables(tables.ptr, coef.ptr, 1))
    state = device.DeviceBuffer((1, 2), np.float64, zero=True)
    out = device.DeviceBuffer((SIZES[-1][0], 1), np.float32)
    w = 2.0 * np.pi * 440.0
    for frames, launches in SIZES:
        if variant == "tone":
            assert lib.pgx_biquad_tone_supported(frames, settle, w, SR, *c) == 1

            def launch():
                device.check(lib.pgx_biquad_tone(out.ptr, 10 ** 9, frames, SR, w, 1.0, 0.0, *c, tables.ptr, settle,
                                                 state.ptr, None))
        else:
            def launch():
                device.check(lib.pgx_biquad_sine(out.ptr, 10 ** 9, frames, SR, w, 1.0, 0.0, coef.ptr, tables.ptr, settle,
                                                 state.ptr, None))

        for _ in range(launches // 2):
            launch()
        e0, e1 = device.Event(), device.Event()
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        device.synchronize()
        us = e1.elapsed_ms_since(e0) / launches * 1e3
        print(json.dumps({"frames": frames, "launches": launches, "us": round(us, 3),
                          "tb_s": round(4.0 * frames / us / 1e6, 3)}), flush=True)


def run(out_dir, passes):
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    with open(os.path.join(out_dir, "c2_tone.jsonl"), "w") as raw:
        for p in range(passes):
            for name in VARIANTS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", name], capture_output=True,
                                   text=True, timeout=240)
                if r.returncode != 0:          # nothing more is started on the device after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"{name}: worker exit {r.returncode}")
                for line in r.stdout.splitlines():
                    if line.startswith("{"):
                        row = dict(json.loads(line), variant=name, **{"pass": p})
                        rows.append(row)
                        raw.write(json.dumps(row) + "\n")
                        raw.flush()
    md = ["# BiquadPE(SinePE) windows in closed form: `pgx_biquad_tone` against the wave-run kernel", "",
          f"µs per launch, median [min – max] of {passes} passes, and TB/s of the median (4 B per frame):", "",
          "| variant | " + " | ".join(f"{f:,} frames".replace(",", " ") for f, _ in SIZES) + " |", "|---|" + "---|" * len(SIZES)]
    med = {}
    for name in VARIANTS:
        cells = []
        for f, _ in SIZES:
            t = sorted(r["us"] for r in rows if r["variant"] == name and r["frames"] == f)
            med[name, f] = statistics.median(t)
            cells.append(f"{med[name, f]:.1f} [{t[0]:.1f} – {t[-1]:.1f}], {4.0 * f / med[name, f] / 1e6:.2f}")
        md.append(f"| {name} | " + " | ".join(cells) + " |")
    md.append("| tone / runs | " + " | ".join(f"{med['tone', f] / med['runs', f]:.3f}" for f, _ in SIZES) + " |")
    path = os.path.join(out_dir, "c2_tone.md")
    rest = ""
    if os.path.exists(path):
        text = open(path).read()
        if MARK in text:
            rest = text.split(MARK, 1)[1]
    with open(path, "w") as f:
        f.write("\n".join(md) + "\n\n" + MARK + rest)
    print("\n".join(md))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "worker":
        worker(sys.argv[2])
    elif mode == "run":
        out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "runs")
        run(out_dir, int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 3)
    else:
        raise SystemExit(__doc__)
