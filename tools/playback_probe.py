"""
Throughput of WavetablePE / TimeWarpPE renders, each graph beside itself with its host-side shortcut switched off:
  wavetable_osc    a 2048-frame sine table read by a ~440 Hz saw (cubic, wrap); off: wavetable_pe.KEEP_TABLE = False
                   (the table window is found by a device min / max + a 16-byte read and rendered on every pull)
  timewarp_scalar  SinePE(220) under rate 1.5 (cubic); off: timewarp_pe.NO_READBACK = False (rate stream + scan +
                   16-byte read, the PE-rate path)
  timewarp_ramp    the same source under a PiecewisePE rate ramp 0.5 -> 2.0: always the PE-rate path, no switch
at 48 000 and 1 000 000 frames per render.  Each row times `steps` contiguous renders of the whole graph between two HIP
events on the library stream (so host gaps -- the read-backs -- count, as they do for a user), after warm-up renders of
the same size; on / off alternate within each repeat.

Then pgx_wavetable alone (cubic, wrap) over uniformly random and over saw indices, table windows of 2 051, 4 003 and
8 003 frames, with the window staged in LDS (PGX_WT_LDS_FLOATS=16384) and gathered from global memory
(PGX_WT_LDS_FLOATS=0): what the staging is worth, per launch.

One JSON line per row and repeat.  Measured values, no gate.
    python tools/playback_probe.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygmu2_amd as pg                                            # noqa: E402
from pygmu2_amd import device, timewarp_pe, wavetable_pe           # noqa: E402

SR = 48000


def graph(kind):
    pg.set_sample_rate(SR)
    if kind == "wavetable_osc":
        table = pg.ArrayPE(np.sin(2 * np.pi * np.arange(2048) / 2048).astype(np.float32))
        saw = pg.LoopPE(pg.PiecewisePE([(0, 0.0), (109, 2048.0)]), 0, 109)
        return pg.WavetablePE(table, saw, pg.InterpolationMode.CUBIC, pg.OutOfBoundsMode.WRAP)
    if kind == "timewarp_scalar":
        return pg.TimeWarpPE(pg.SinePE(220.0), 1.5, pg.InterpolationMode.CUBIC)
    rate = pg.PiecewisePE([(0, 0.5), (200_000_000, 2.0)], extend_mode=pg.ExtendMode.HOLD_BOTH)
    return pg.TimeWarpPE(pg.SinePE(220.0), rate, pg.InterpolationMode.CUBIC)


def timed(pe, frames, steps, warmup=5):
    renderer = pg.NullRenderer(sample_rate=SR)
    renderer.set_source(pe)
    renderer.start()
    pos = 0
    for _ in range(warmup):
        pe.render(pos, frames)
        pos += frames
    device.synchronize()
    t0, t1 = device.Event(), device.Event()
    t0.record()
    for _ in range(steps):
        pe.render(pos, frames)
        pos += frames
    t1.record()
    ms = t1.elapsed_ms_since(t0)
    renderer.stop()
    return ms / steps


def kernel_rows():
    lib = device.ensure_init()
    rng = np.random.default_rng(0)
    for table_len in (2048, 4000, 8000):
        window = device.DeviceBuffer.from_host(rng.standard_normal((table_len + 3, 1)).astype(np.float32))
        for frames, steps in ((48_000, 4000), (1_000_000, 1000)):
            saw = (np.arange(frames) * (table_len / 109.0)) % table_len
            for name, host in (("random", rng.uniform(0, table_len, frames)), ("saw", saw)):
                index = device.DeviceBuffer.from_host(host.astype(np.float32).reshape(-1, 1))
                out = device.DeviceBuffer((frames, 1), np.float32)

                def launch():
                    device.check(lib.pgx_wavetable(out.ptr, index.ptr, frames, window.ptr, -1, table_len + 3, 1, 1, 2,
                                                   1, 0.0, float(table_len)), "pgx_wavetable")
                for repeat in range(3):
                    for staged in (True, False):
                        os.environ["PGX_WT_LDS_FLOATS"] = "16384" if staged else "0"
                        for _ in range(10):
                            launch()
                        device.synchronize()
                        t0, t1 = device.Event(), device.Event()
                        t0.record()
                        for _ in range(steps):
                            launch()
                        t1.record()
                        us = t1.elapsed_ms_since(t0) * 1e3 / steps
                        print(json.dumps({"row": "pgx_wavetable", "table": table_len, "indices": name, "frames": frames,
                                          "lds": "staged" if staged else "global", "repeat": repeat,
                                          "us_per_launch": round(us, 3)}), flush=True)
    os.environ.pop("PGX_WT_LDS_FLOATS", None)


def main():
    switches = {"wavetable_osc": (wavetable_pe, "KEEP_TABLE"), "timewarp_scalar": (timewarp_pe, "NO_READBACK"),
                "timewarp_ramp": None}
    for kind, switch in switches.items():
        for frames, steps in ((48_000, 2000), (1_000_000, 400)):
            for repeat in range(3):
                for on in ((True, False) if switch else (True,)):
                    if switch:
                        setattr(switch[0], switch[1], on)
                    try:
                        ms = timed(graph(kind), frames, steps)
                    finally:
                        if switch:
                            setattr(switch[0], switch[1], True)
                    print(json.dumps({"row": kind, "frames": frames, "shortcut": "on" if on else "off",
                                      "repeat": repeat, "steps": steps, "ms_per_render": round(ms, 5),
                                      "frames_per_s": round(frames / (ms * 1e-3))}), flush=True)
    kernel_rows()


if __name__ == "__main__":
    main()
