"""The closed form of PortamentoPE's pitch line restated in numpy, for the host test, the GPU tests and the fixture
generator (tools/gen_golden_portamento.py), which holds it to the reference's renders bit for bit.

Notes (pitch, start, duration) sorted by start (stable), R = max(1, round(max_ramp_seconds * sample_rate)).  For N >= 2
notes ramp i (0 .. N-2): from pitch[i] to pitch[i+1], at = int(start[i+1]), len = max(1, min(R, round(duration[i+1] *
ramp_fraction))).  Ramp i owns [at_i, at_{i+1}), the last ramp [at_{N-2}, +inf), the first also everything before at_0;
an empty interval owns nothing.  At frame s of ramp i, x = s - at_i: x <= 0 -> from; x >= len -> to; else from + (to -
from) * (float64(x) / float64(len)), rounded once to float32.  One note: its pitch everywhere -- written as one ramp from
the pitch to the pitch, which is that.  Every channel carries the same value."""

import numpy as np

FIXTURE = "portamento"


def table(notes, max_ramp_seconds, ramp_fraction, sample_rate):
    """-> (at int64, len int64, from float64, to float64), one row per ramp."""
    order = sorted(range(len(notes)), key=lambda k: notes[k][1])          # stable, as sorted(notes, key=...) is
    pitch = np.array([notes[k][0] for k in order], np.float64)
    start = [notes[k][1] for k in order]
    duration = [notes[k][2] for k in order]
    if len(order) == 1:
        return np.array([int(start[0])], np.int64), np.ones(1, np.int64), pitch.copy(), pitch.copy()
    longest = max(1, int(round(max_ramp_seconds * sample_rate)))
    at = np.array([int(s) for s in start[1:]], np.int64)
    length = np.array([max(1, min(longest, int(round(d * ramp_fraction)))) for d in duration[1:]], np.int64)
    return at, length, pitch[:-1].copy(), pitch[1:].copy()


def case_table(case):
    return table([tuple(n) for n in case["notes"]], case["max_ramp_seconds"], case["ramp_fraction"], case["sr"])


def line(tab, start, n, channels=1):
    """Frames [start, start + n) of the line of a table -> float32 (n, channels)."""
    at, length, v0, v1 = tab
    s = start + np.arange(n, dtype=np.int64)
    j = np.maximum(np.searchsorted(at, s, side="right"), 1) - 1           # the last ramp that has begun; never before 0
    x = s - at[j]
    with np.errstate(invalid="ignore"):
        glide = v0[j] + (v1[j] - v0[j]) * (x.astype(np.float64) / length[j].astype(np.float64))
    value = np.where(x <= 0, v0[j], np.where(x >= length[j], v1[j], glide)).astype(np.float32)
    return np.repeat(value[:, None], channels, axis=1)


def owners(tab, start, n):
    """The ramp that owns each frame of [start, start + n)."""
    s = start + np.arange(n, dtype=np.int64)
    return np.maximum(np.searchsorted(tab[0], s, side="right"), 1) - 1


def pack(tables):
    """Several lines' tables as pgx_portamento's arrays -> (at, len, from, to, offsets int32 [lines + 1])."""
    offsets = np.concatenate(([0], np.cumsum([t[0].shape[0] for t in tables]))).astype(np.int32)
    return tuple(np.concatenate([t[k] for t in tables]) for k in range(4)) + (offsets,)


def build(pg, case):
    return pg.PortamentoPE([tuple(n) for n in case["notes"]], max_ramp_seconds=case["max_ramp_seconds"],
                           ramp_fraction=case["ramp_fraction"], channels=case["channels"])
