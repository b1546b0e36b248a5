"""
What a block of RandomSelectPE costs with the restart bank on (a scan of the trigger, one render per distinct candidate,
one gather) and off (the composed path: the trigger block read back, one render and one copy per event -- the code
TriggerRestartPE ran before the bank existed).  The three graphs of the reference's examples/random_select_eg.py at
48 kHz:
  sines      six weighted SinePE candidates                                   (demo 1)
  one_osc    SinePE(frequency=RandomSelectPE(six weighted ConstantPE))        (demo 2)
  slices     ten SlicePE cuts of one 114 541-frame recording, here an ArrayPE (demo 3)
each under a 10 Hz and a 1 kHz PeriodicTrigger, pulled in blocks of 4 800 and of 48 000 frames.

Rows: microseconds of wall time per block (host clock around sequential renders in a started NullRenderer, the device
synchronised at both ends; at least 0.25 s or 5 blocks per timing), a warm-up repeat and three timed ones, on and off
alternating within a repeat.  In the warm-up repeat the first blocks of both paths are compared: `same` must be true.
The step runs in a child process under a time limit.  One JSON line per timing on stdout (and in --out FILE).
Measured values, no gate.
    python tools/random_select_probe.py [--out profiles/random_select_probe.jsonl]
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
LIMIT = 900                  # seconds allowed for the step
MIN_SECONDS = 0.25
CUTS = (0, 13811, 20882, 35331, 42732, 57006, 71456, 78857, 93130, 100355, 114541)
PITCHES = (55, 57, 62, 64, 69, 71)


def graph(pg, name, hz):
    trigger = pg.PeriodicTrigger(hz=hz)
    freqs = [float(pg.pitch_to_freq(p)) for p in PITCHES]
    if name == "sines":
        return pg.RandomSelectPE(trigger, [pg.SinePE(frequency=f, amplitude=0.3) for f in freqs],
                                 weights=[0.1, 0.4, 0.2, 0.3, 0.4, 0.4], seed=1234)
    if name == "one_osc":
        chooser = pg.RandomSelectPE(trigger, [pg.ConstantPE(f) for f in freqs], weights=[0.1, 0.4, 0.2, 0.3, 0.4, 0.1],
                                    seed=1234)
        return pg.SinePE(frequency=chooser, amplitude=0.3)
    rng = np.random.default_rng(7)
    recording = pg.ArrayPE(rng.uniform(-1.0, 1.0, (CUTS[-1], 1)).astype(np.float32))
    return pg.RandomSelectPE(trigger, [pg.SlicePE(recording, a, b - a) for a, b in zip(CUTS, CUTS[1:])], seed=1234)


def timed(pg, device, pe, block, blocks):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(pe)
    r.start()
    device.synchronize()
    t0 = time.perf_counter()
    for i in range(blocks):
        pe.render(i * block, block)
    device.synchronize()
    seconds = time.perf_counter() - t0
    r.stop()
    return seconds


def step():
    import pygmu2_amd as pg
    from pygmu2_amd import device, restart_bank
    pg.set_sample_rate(SR)
    for name in ("sines", "one_osc", "slices"):
        for hz in (10.0, 1000.0):
            for block in (4800, 48000):
                counts, same = {}, None
                for repeat in range(4):                  # repeat 0 warms up, sizes the timings and compares the samples
                    firsts = {}
                    for bank in (True, False):
                        restart_bank.set_enabled(bank)
                        pe = graph(pg, name, hz)
                        if repeat == 0:
                            per = timed(pg, device, pe, block, 2) / 2
                            counts[bank] = int(min(400, max(5, math.ceil(MIN_SECONDS / max(per, 1e-6)))))
                            firsts[bank] = np.array(pe.render(0, block).data)
                            pe = graph(pg, name, hz)
                        seconds = timed(pg, device, pe, block, counts[bank])
                        if repeat == 0 and len(firsts) == 2:
                            same = bool(np.array_equal(firsts[True], firsts[False]))
                        print(json.dumps({"graph": name, "trigger_hz": hz, "block": block, "bank": bank, "repeat": repeat,
                                          "warm_up": repeat == 0, "blocks": counts[bank], "same": same,
                                          "us_per_block": round(seconds / counts[bank] * 1e6, 2)}), flush=True)
    restart_bank.set_enabled(True)


def main():
    if "--step" in sys.argv:
        step()
        return 0
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None
    import threading
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step"], stdout=subprocess.PIPE, text=True)
    watchdog = threading.Timer(LIMIT, p.kill)
    watchdog.start()
    try:
        for line in p.stdout:                            # rows as they come
            sys.stdout.write(line)
            sys.stdout.flush()
            if out:
                out.write(line)
                out.flush()
        status = p.wait()
    finally:
        watchdog.cancel()
    if status != 0:
        print(f"the step ended with status {status} (time limit {LIMIT} s); stopping", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
