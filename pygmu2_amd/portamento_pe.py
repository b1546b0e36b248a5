"""
PortamentoPE: the pitch line of a monophonic voice (portamento_pe.py:23-285) -- each note's pitch held, with a short
linear glide from the previous pitch at every note's start.  The reference composes the line from one PiecewisePE ramp
per transition, each under a CropPE and a DelayPE, summed by a MixPE; exactly one of them is non-zero at any frame.
Here the line is one table of ramps and one launch (pgx_portamento).

The closed form (`ramp_table`): the notes (pitch, start, duration) sorted by start, R = max(1, round(max_ramp_seconds *
sample_rate)); for N >= 2 notes ramp i (0 .. N-2) glides from pitch[i] to pitch[i+1], begins at int(start[i+1]) and
lasts max(1, min(R, round(duration[i+1] * ramp_fraction))) frames.  Ramp i owns the frames from its beginning to the
next ramp's, the last one every frame from its beginning on, the first one also every frame before.  One note is its
pitch at every frame.  Extent: infinite.

Two departures from what the reference renders (once its SequencePE call is made to accept `channels`), both towards
its own docstring: with three or more notes the reference returns zeros for a request that ends at or before the
second note's start (and the held first pitch for one that straddles it) -- here the first pitch is held for all
frames before the second note; and where two notes share a start the reference renders 0 before that start -- here the
earlier of the two owns no frame and the line goes on.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from ._kernels import DeviceBuffer, check, lib, new_output
from .snippet import Snippet
from .source_pe import SourcePE


def ramp_table(notes: Sequence[Tuple[float, int, int]], max_ramp_seconds: float, ramp_fraction: float,
               sample_rate: int):
    """The ramps of a line whose notes are sorted by start, as pgx_portamento's four columns: beginnings and lengths
    (int64), start and end pitches (float64).  One note: one ramp from its pitch to its pitch."""
    if len(notes) == 1:
        pitch, start, _ = notes[0]
        return (np.array([int(start)], np.int64), np.array([1], np.int64),
                np.array([pitch], np.float64), np.array([pitch], np.float64))
    longest = max(1, int(round(max_ramp_seconds * sample_rate)))
    at, length, v0, v1 = [], [], [], []
    for (prev_pitch, _, _), (pitch, start, duration) in zip(notes[:-1], notes[1:]):
        at.append(int(start))
        length.append(max(1, min(longest, int(round(duration * ramp_fraction)))))
        v0.append(prev_pitch)
        v1.append(pitch)
    return np.array(at, np.int64), np.array(length, np.int64), np.array(v0, np.float64), np.array(v1, np.float64)


class PortamentoPE(SourcePE):
    _READ_AHEAD_SAFE = True

    def __init__(self, notes: List[Tuple[float, int, int]], max_ramp_seconds: float = 0.1,
                 ramp_fraction: float = 0.3, channels: int = 1):
        if not notes:
            raise ValueError("PortamentoPE: notes list cannot be empty")
        if max_ramp_seconds < 0:
            raise ValueError(f"PortamentoPE: max_ramp_seconds must be non-negative (got {max_ramp_seconds})")
        if not (0.0 <= ramp_fraction <= 1.0):
            raise ValueError(f"PortamentoPE: ramp_fraction must be between 0 and 1 (got {ramp_fraction})")
        if channels < 1:
            raise ValueError(f"PortamentoPE: channels must be >= 1 (got {channels})")
        self._notes = sorted(notes, key=lambda x: x[1])
        self._max_ramp_seconds = float(max_ramp_seconds)
        self._ramp_fraction = float(ramp_fraction)
        self._channels = int(channels)
        # the sample rate is read here, as the reference builds its ramps at construction
        self._table = ramp_table(self._notes, self._max_ramp_seconds, self._ramp_fraction, self.sample_rate)
        self._table_dev: Tuple[DeviceBuffer, ...] | None = None       # uploaded on the first render

    @property
    def notes(self) -> List[Tuple[float, int, int]]:
        """The (pitch, sample_index, duration) tuples, sorted by sample_index."""
        return self._notes.copy()

    max_ramp_seconds = property(lambda self: self._max_ramp_seconds)
    ramp_fraction = property(lambda self: self._ramp_fraction)

    def channel_count(self) -> int:
        return self._channels

    def _render(self, start: int, duration: int) -> Snippet:
        if self._table_dev is None:
            offsets = np.array([0, self._table[0].shape[0]], np.int32)
            self._table_dev = tuple(DeviceBuffer.from_host(column) for column in self._table + (offsets,))
        at, length, v0, v1, offsets = self._table_dev
        out = new_output(duration, self._channels)
        check(lib().pgx_portamento(out.ptr, duration * self._channels, 1, start, duration, self._channels, at.ptr,
                                   length.ptr, v0.ptr, v1.ptr, offsets.ptr), "pgx_portamento")
        return Snippet(start, out)

    def __repr__(self) -> str:
        return (f"PortamentoPE({len(self._notes)} notes, max_ramp_seconds={self._max_ramp_seconds}, "
                f"ramp_fraction={self._ramp_fraction}, channels={self._channels})")
