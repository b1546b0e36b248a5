"""
What PortamentoPE's kernel costs, in one run:
  kernel     pgx_portamento, one line of 4, 64, 512 and 1 024 notes, 1 024, 48 000, 2^22 and 2^25 frames per launch, one
             channel, beside pgx_fill on the same buffer (the same 4 B per frame written and nothing computed): microseconds
             per launch and the achieved store rate of both.  The lines that the kernel reads from LDS (up to 512 ramps) also
             with the table read from global memory (PGX_PORTA_LDS_RAMPS=0).  HIP events on the library stream around at
             least 0.25 s of repeated launches after warm-up, three repeats with the sides alternating.
  graph      PortamentoPE.render against the graph the reference composes the line from, built of this package's own
             PiecewisePE, CropPE, DelayPE and MixPE (one ramp per transition, cropped to its interval, delayed to its note,
             mixed): the same notes and block lengths, the blocks between the second note's start and the melody's end
             walked round and round, read-ahead and look-ahead windows off, host clock around renders that each end in a
             device synchronise.  The first block of both is compared to the bit before anything is timed.

Every step runs in a child process of its own under a time limit; a step that fails ends the run.  One JSON line per
row and repeat on stdout (and in --out FILE).  Measured values, no gate.
    python tools/portamento_probe.py [--out profiles/portamento_probe.jsonl]
One step alone:
    python tools/portamento_probe.py --step kernel|graph
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
NOTES = (4, 64, 1024)                                # the graph step's lines
KERNEL_NOTES = (4, 64, 512, 1024)
BLOCKS = (1024, 48_000)
KERNEL_BLOCKS = BLOCKS + (1 << 22, 1 << 25)
LDS_RAMPS = 512                                      # kPortaLdsRamps
NOTE_FRAMES = 6000                                   # an eighth of a second per note
STEPS = {"kernel": 240, "graph": 300}                # seconds allowed per step
MIN_SECONDS = 0.25
LDS_ENV = "PGX_PORTA_LDS_RAMPS"


def emit(**row):
    print(json.dumps(row), flush=True)


def melody(count):
    """`count` abutting notes of NOTE_FRAMES frames, pitches that wander over two octaves."""
    rng = np.random.default_rng(count)
    pitch = 60.0 + np.round(rng.uniform(-12.0, 12.0, count), 2)
    return [(float(p), k * NOTE_FRAMES, NOTE_FRAMES) for k, p in enumerate(pitch)]


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


def step_kernel():
    from pygmu2_amd import device
    from pygmu2_amd.portamento_pe import ramp_table
    lib = device.ensure_init()
    for count in KERNEL_NOTES:
        table = ramp_table(melody(count), 0.1, 0.3, SR)
        cols = [device.DeviceBuffer.from_host(c) for c in table + (np.array([0, count - 1], np.int32),)]
        for n in KERNEL_BLOCKS:
            out = device.DeviceBuffer((n, 1), np.float32)
            # a block from the middle of the line: it crosses n / NOTE_FRAMES notes
            start = (count // 2) * NOTE_FRAMES - n // 2

            def glide():
                device.check(lib.pgx_portamento(out.ptr, n, 1, start, n, 1, *(c.ptr for c in cols)), "pgx_portamento")

            def glide_global():
                os.environ[LDS_ENV] = "0"
                try:
                    glide()
                finally:
                    del os.environ[LDS_ENV]

            sides = {"pgx_portamento": glide, "pgx_fill": lambda: device.check(lib.pgx_fill(out.ptr, n, 0.5), "pgx_fill")}
            if count - 1 <= LDS_RAMPS:
                sides["pgx_portamento, table in global memory"] = glide_global
            for repeat in range(3):
                for name, launch in sides.items():
                    us, steps = time_launches(device, launch)
                    emit(row="kernel", kernel=name, notes=count, frames=n, repeat=repeat, launches=steps,
                         us_per_launch=round(us, 3), write_gb_per_s=round(4.0 * n / us * 1e-3, 2))


def composed(pg, notes, max_ramp_seconds=0.1, ramp_fraction=0.3):
    """The line as the reference composes it (three or more notes), of this package's classes."""
    longest = max(1, int(round(max_ramp_seconds * SR)))
    last = len(notes) - 2
    parts = []
    for i in range(len(notes) - 1):
        (p0, _, _), (p1, at, duration) = notes[i], notes[i + 1]
        ramp = pg.PiecewisePE([(0, p0), (max(1, min(longest, int(round(duration * ramp_fraction)))), p1)],
                              extend_mode=pg.ExtendMode.HOLD_BOTH)
        if i == last:
            ramp = pg.CropPE(ramp, 0, None)
        else:
            ramp = pg.CropPE(ramp, 0, notes[i + 2][1] - at, pg.ExtendMode.HOLD_FIRST if i == 0 else pg.ExtendMode.ZERO)
        parts.append(pg.DelayPE(ramp, delay=at))
    return pg.MixPE(*parts)


def step_graph():
    import pygmu2_amd as pg
    from pygmu2_amd import device, look_ahead, read_ahead
    pg.set_sample_rate(SR)
    look_ahead.set_enabled(False)          # consecutive pulls would be served from windows: time renders
    read_ahead.set_enabled(False)
    for count in NOTES:
        notes = melody(count)
        first = notes[1][1]
        for n in BLOCKS:
            sides = {"PortamentoPE": pg.PortamentoPE(notes), "composed graph": composed(pg, notes)}
            blocks = {}
            for name, pe in sides.items():
                r = pg.NullRenderer(sample_rate=SR)
                r.set_source(pe)
                r.start()
                blocks[name] = np.array(pe.render(first, n).data)
            same = bool(np.array_equal(blocks["PortamentoPE"].view(np.uint32), blocks["composed graph"].view(np.uint32)))
            inside = max(1, (count * NOTE_FRAMES - first) // n)     # blocks that lie inside the melody: walked round and round
            for repeat in range(3):
                for name, pe in sides.items():
                    for i in range(2):
                        pe.render(first + (i % inside) * n, n)
                    device.synchronize()
                    renders, t = 0, time.perf_counter()
                    while time.perf_counter() - t < MIN_SECONDS or renders < 3:
                        pe.render(first + (renders % inside) * n, n)
                        device.synchronize()
                        renders += 1
                    dt = time.perf_counter() - t
                    emit(row="graph", side=name, notes=count, frames=n, repeat=repeat, renders=renders, same_bits=same,
                         us_per_block=round(dt * 1e6 / renders, 1))


def main():
    table = {"kernel": step_kernel, "graph": step_graph}
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
