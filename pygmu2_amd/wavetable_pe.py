"""
WavetablePE: out[t] = wavetable[indexer[t]] with a fractional, signal-valued index (wavetable_pe.py:32-178).

The index stream stays on the device: one launch (pgx_wavetable) widens it to float64, applies the
out-of-bounds rule (wrap / clamp / zero) and interpolates, linear or Catmull-Rom, through the device function
DelayPE's lookup uses, in the reference's operation order -- the output is the reference's bit for bit.

A table with a finite extent over a pure sub-graph is rendered once, as the window [start - 1, end + 2), and kept
in HBM; no index range is read back.  That is exact: after wrap / clamp every index lies inside the extent, in
zero mode every index outside it is masked, frames outside the extent are 0 in whichever window they are
rendered, and the reference's window clipping only ever reaches a neighbour whose weight is 0.  Unbounded,
impure or very large tables go DelayPE's way: min / max of the processed indices on the device
(pgx_wavetable_range), 16 bytes read back, that window rendered.
"""

from __future__ import annotations

from enum import Enum

import numpy as np

from ._kernels import DeviceBuffer, check, lib, new_output
from .delay_pe import InterpolationMode
from .extent import Extent
from .loop_pe import _subtree_pure
from .processing_element import ProcessingElement
from .snippet import Snippet

KEEP_TABLE = True                        # module switch: False renders the table window on every pull (measurements)
KEPT_TABLE_MAX_BYTES = 4 << 20           # larger tables are not kept: their window follows the indices


class OutOfBoundsMode(Enum):
    ZERO = "zero"
    CLAMP = "clamp"
    WRAP = "wrap"


_MODE_CODE = {"zero": 0, "clamp": 1, "wrap": 2}


class WavetablePE(ProcessingElement):
    def __init__(self, wavetable: ProcessingElement, indexer: ProcessingElement,
                 interpolation: InterpolationMode = InterpolationMode.LINEAR,
                 out_of_bounds: OutOfBoundsMode = OutOfBoundsMode.ZERO):
        self._wavetable = wavetable
        self._indexer = indexer
        self._interpolation = interpolation
        self._out_of_bounds = out_of_bounds
        self._kept: Snippet | None = None                 # the table window, under a pure sub-graph only
        self._range_dev: DeviceBuffer | None = None
        self.d2h_reads = 0                                # device-to-host copies this PE has issued

    wavetable = property(lambda self: self._wavetable)
    indexer = property(lambda self: self._indexer)
    interpolation = property(lambda self: self._interpolation)
    out_of_bounds = property(lambda self: self._out_of_bounds)

    def inputs(self) -> list[ProcessingElement]:
        return [self._wavetable, self._indexer]

    # pure, but not _READ_AHEAD_SAFE: with a table that is not kept, a read-ahead window would size the table render from
    # the indices of the whole window instead of each block's, and the reference's window clipping is per render
    def is_pure(self) -> bool:
        return True

    def channel_count(self) -> int | None:
        return self._wavetable.channel_count()

    def _compute_extent(self) -> Extent:
        return self._indexer.extent()

    def _drop_table(self) -> None:
        self._kept = None

    _on_start = _on_stop = _drop_table

    def _keeps_table(self, wt_len: int) -> bool:
        if not KEEP_TABLE or wt_len < 1:
            return False
        ch = self._wavetable.channel_count() or 1
        return (wt_len + 3) * ch * 4 <= KEPT_TABLE_MAX_BYTES and _subtree_pure(self._wavetable)

    def _render(self, start: int, duration: int) -> Snippet:
        _, index_buf = self._control_stream(self._indexer, start, duration)
        cubic = getattr(self._interpolation, "value", self._interpolation) == "cubic"
        mode = _MODE_CODE[getattr(self._out_of_bounds, "value", self._out_of_bounds)]
        ext = self._wavetable.extent()
        finite = ext.start is not None and ext.end is not None
        wt_start, wt_end = (float(ext.start), float(ext.end)) if finite else (0.0, 0.0)
        L = lib()
        if finite and self._keeps_table(ext.end - ext.start):
            window = self._kept
            if window is None:
                window = self._kept = self._wavetable.render(ext.start - 1, ext.end - ext.start + 3)
            win_start, win_len = ext.start - 1, ext.end - ext.start + 3
        else:
            if self._range_dev is None:
                self._range_dev = DeviceBuffer((2,), np.float64)
            check(L.pgx_wavetable_range(self._range_dev.ptr, index_buf.ptr, duration, mode, int(finite), wt_start,
                                        wt_end), "pgx_wavetable_range")
            idx_min, idx_max = (float(v) for v in self._range_dev.to_host())
            self.d2h_reads += 1
            if not (np.isfinite(idx_min) and np.isfinite(idx_max)):
                raise ValueError("WavetablePE: index stream contains non-finite values")
            margin = 2 if cubic else 1
            win_start = int(np.floor(idx_min)) - (margin - 1)
            win_len = int(np.ceil(idx_max)) + margin - win_start
            window = self._wavetable.render(win_start, win_len)
        ch = window.channels
        out = new_output(duration, ch)
        check(L.pgx_wavetable(out.ptr, index_buf.ptr, duration, window.dev.ptr, win_start, win_len, ch, int(cubic),
                              mode, int(finite), wt_start, wt_end), "pgx_wavetable")
        return Snippet(start, out)

    def __repr__(self) -> str:
        return (f"WavetablePE(wavetable={type(self._wavetable).__name__}, indexer={type(self._indexer).__name__}, "
                f"interpolation={self._interpolation.value}, out_of_bounds={self._out_of_bounds.value})")
