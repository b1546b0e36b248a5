"""
Throughput of KarplusStrongPE / AnalogOscPE renders (the suite protocol of tools/bench_suite.py: 5 warm-up + 50 timed
renders of 44 100 frames; "sync" waits for every render, "pipe" only for the last).  Prints one JSON line per row with
Msamples/s and the fraction of the binding roof:
  KarplusStrongPE: the dependent float32 multiply + subtract per frame (2 x ~4 cycles at 2.4 GHz, per string) or, for
                   batches that fill the chip, the HBM roof of the 4 B written per string-frame;
  AnalogOscPE:     the HBM roof (5.3 TB/s) of the bytes each frame moves (4 B written, + 8 B of streams read for the
                   stateful form, x the passes that touch them).
    python tools/sources_probe.py
"""

from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygmu2_amd as pg                                   # noqa: E402
from pygmu2_amd import device                             # noqa: E402
from pygmu2_amd.device import DeviceBuffer                # noqa: E402

SR = 44100
HBM = 5.3e12
CLOCK = 2.4e9


def timed(fn, steps=50, warmup=5, sync=True):
    for _ in range(warmup):
        fn()
    device.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        if sync:
            device.synchronize()
    device.synchronize()
    return (time.perf_counter() - t0) / steps


def ks_bank(batch, frames):
    lib = device.ensure_init()
    rng = np.random.default_rng(0)
    freqs = np.exp(rng.uniform(np.log(55.0), np.log(1760.0), batch)) if batch > 1 else np.array([440.0])
    ns = np.maximum(2, np.floor(SR / freqs)).astype(np.int64)
    offs = np.concatenate(([0], np.cumsum(ns)))
    p = np.zeros(batch, dtype=device.KS_PARAMS)
    p["line_offset"], p["n"], p["rho"], p["c"] = offs[:-1], ns, 0.996, 0.5
    pb = DeviceBuffer.from_host(p)
    lines = DeviceBuffer.from_host(rng.standard_normal(int(offs[-1])).astype(np.float32) * 0.3)
    st = DeviceBuffer((batch,), device.KS_STATE, zero=True)
    out = DeviceBuffer((batch, frames), np.float32)
    pos = [0]

    def fn():
        device.check(lib.pgx_karplus_strong(out.ptr, frames, batch, pos[0], frames, 1, pb.ptr, lines.ptr, st.ptr,
                                            int(ns.max())), "pgx_karplus_strong")
        pos[0] += frames
    return fn


def osc_fn(kind, frames):
    pg.set_sample_rate(SR)
    if kind == "pure_rect":
        pe = pg.AnalogOscPE(110.3, 0.3, "rectangle")
    elif kind == "pure_saw":
        pe = pg.AnalogOscPE(110.3, 0.3, "sawtooth")
    else:
        duty = pg.TransformPE(pg.SinePE(frequency=0.25), func=pg.transforms.Affine(0.45, 0.5))
        pe = pg.AnalogOscPE(110.3, duty, "rectangle")
    pos = [0]

    def fn():
        pe._render(pos[0], frames)      # the PE's own launches (no read-/look-ahead window)
        pos[0] += frames
    return fn


def main():
    rows = []
    for batch in (1, 64, 1024, 4096):
        fn = ks_bank(batch, SR)
        for sync in (True, False):
            t = timed(fn, sync=sync)
            ms = batch * SR / t / 1e6
            roof_chain = CLOCK / 8.0 * batch                  # string-frames / s on the serial chain
            roof = min(roof_chain, HBM / 4.0)
            rows.append({"row": f"ks_batch{batch}", "mode": "sync" if sync else "pipe", "ms": t * 1e3,
                         "msamples_s": ms, "roof_fraction": ms * 1e6 / roof})
    for kind, bytes_per in (("pure_rect", 4.0), ("pure_saw", 8.0), ("stateful_pe_duty", 4.0 + 3 * 4.0)):
        for frames in (SR, 1 << 24):
            fn = osc_fn(kind, frames)
            for sync in (True, False):
                t = timed(fn, steps=50 if frames == SR else 10, sync=sync)
                ms = frames / t / 1e6
                rows.append({"row": f"osc_{kind}_{frames}", "mode": "sync" if sync else "pipe", "ms": t * 1e3,
                             "msamples_s": ms, "roof_fraction": ms * 1e6 * bytes_per / HBM})
    for r in rows:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
