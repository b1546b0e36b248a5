#!/usr/bin/env python3
"""Host time per look-ahead window of a long C2 stream (GPU box): every pull of 1 000 000 frames timed on the host, split into
the pulls that open a window and the pulls served from one; per window = one opening + (blocks - 1) served pulls, to set
beside the window kernel's device time.  The stream is synchronised every 40 windows, outside the timed pulls, so the
host never waits for a full queue.

    python tools/c2_window_host.py [--windows 400] [--profile]

The window size is the stream's own (pgx_biquad_tone_window_frames, or PGX_TONE_WINDOW_FRAMES / PGX_LOOK_AHEAD_FRAMES).
--profile: cProfile over the same stream, the 25 entries with the largest cumulative time.
"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import pygmu2_amd as pg
from pygmu2_amd import device, look_ahead

windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 400
frames = 1_000_000


def stream(pe, pos, count, record):
    clock, stats = time.perf_counter, look_ahead.STATS
    keep, opened = None, 0
    while opened < count:
        before = stats["windows"]
        t0 = clock()
        keep = pe.render(pos, frames)
        dt = clock() - t0
        pos += frames
        if stats["windows"] != before:
            opened += 1
            record.append((True, dt, (stats["window_frames"] - record_frames[0]) // frames))
            record_frames[0] = stats["window_frames"]
            if opened % 40 == 0:
                device.synchronize()
        else:
            record.append((False, dt, 0))
    return pos


pe, r = bench.c2_graph(pg)
record_frames = [look_ahead.STATS["window_frames"]]
pos = stream(pe, 0, 60, [])                     # slow start and a warm process
device.synchronize()
record = []
record_frames[0] = look_ahead.STATS["window_frames"]
if "--profile" in sys.argv:
    import cProfile, pstats
    pr = cProfile.Profile()
    pr.enable()
    stream(pe, pos, windows, record)
    pr.disable()
    device.synchronize()
    pstats.Stats(pr).sort_stats("cumulative").print_stats(25)
else:
    stream(pe, pos, windows, record)
    device.synchronize()
opens = sorted(dt for o, dt, _ in record if o)
serves = sorted(dt for o, dt, _ in record if not o)
blocks = statistics.median(b for o, _, b in record if o)
med = lambda v: v[len(v) // 2] * 1e6
print(f"windows of {blocks} blocks: opening median {med(opens):.2f} us (min {opens[0] * 1e6:.2f}), served pull median "
      f"{med(serves):.3f} us (min {serves[0] * 1e6:.3f}); host per window {med(opens) + (blocks - 1) * med(serves):.2f} us "
      f"= {(med(opens) + (blocks - 1) * med(serves)) / blocks:.3f} us per step")
r.stop()
