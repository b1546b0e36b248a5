"""
TimeWarpPE: the "tape head" (timewarp_pe.py:38-195): pos[n+1] = pos[n] + rate[n], the source read at pos by
linear or Catmull-Rom interpolation, 0 where the head is outside the source's extent.  Stateful: the head is
carried between renders and goes back to 0 on start / stop / reset_state().  A gap between two renders does
not move it -- the reference does not look at `start` either.

Scalar rate: positions are pos + i * rate, computed in the lookup kernel itself (pgx_timewarp); they are
monotone, so the host sizes the source window from the two end positions (the same float64 expression), with one
guard frame either side, and nothing is read back.  The head is a host float.  For rates whose multiples are
exact in float64 this is the reference's np.cumsum bit for bit; otherwise it is the correctly rounded product
where the reference accumulates one rounding per frame.

PE rate: a float64 scan of the rate stream over workgroup segments (pgx_timewarp_scan) adds the device-resident
head, leaves the positions and their min / max on the device and advances the head; the host reads the 16 bytes
of min / max to size the source window, as DelayPE does, and pgx_timewarp reads the source at the positions.
"""

from __future__ import annotations

import numpy as np

from . import device
from ._kernels import DeviceBuffer, check, lib, new_output
from .delay_pe import InterpolationMode
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet

# module switch for measurements: False sends a scalar rate down the PE-rate path (scan + 16-byte read), as a float32
# stream like any rendered rate -- so only rates that float32 holds exactly give the same output there
NO_READBACK = True

_WORKSPACE_DOUBLES = device.TIMEWARP_WORKSPACE_DOUBLES


class TimeWarpPE(ProcessingElement):
    def __init__(self, source: ProcessingElement, rate=1.0,
                 interpolation: InterpolationMode = InterpolationMode.LINEAR):
        self._source = source
        self._rate = rate
        self._rate_is_pe = isinstance(rate, ProcessingElement)
        self._interpolation = interpolation
        self._pos = 0.0                                   # the head under a scalar rate
        self._state: DeviceBuffer | None = None           # the head under a PE rate: {pos}
        self._range_dev: DeviceBuffer | None = None
        self._workspace: DeviceBuffer | None = None
        self._positions: DeviceBuffer | None = None
        self._const_rate: DeviceBuffer | None = None
        self._last_render_end: int | None = None
        self.d2h_reads = 0                                # device-to-host copies this PE has issued

    source = property(lambda self: self._source)
    rate = property(lambda self: self._rate)
    interpolation = property(lambda self: self._interpolation)

    def inputs(self) -> list[ProcessingElement]:
        return [self._source, self._rate] if self._rate_is_pe else [self._source]

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int | None:
        return self._source.channel_count()

    def _compute_extent(self) -> Extent:
        if self._rate_is_pe:
            return self._rate.extent()
        src = self._source.extent()
        if src.start is None or src.end is None:
            return Extent(None, None)
        src_start, src_end = float(src.start), float(src.end)
        r = float(self._rate)
        p0 = 0.0
        if r == 0.0:
            # the head stands still: a constant for ever if it stands inside the source, else nothing
            return Extent(None, None) if src_start <= p0 < src_end else Extent(0, 0)
        if r > 0.0:
            n_start = int(np.ceil((src_start - p0) / r)) if src_start > p0 else 0
            n_end = int(np.ceil((src_end - p0) / r))
            n_start = max(0, n_start)
            return Extent(n_start, max(n_start, n_end))
        n_start = max(0, int(np.floor((src_end - p0) / r)) + 1)
        n_end = int(np.floor((src_start - p0) / r)) + 1
        return Extent(n_start, max(n_start, n_end))

    def _rewind(self) -> None:
        self._pos = 0.0
        self._last_render_end = None
        if self._state is not None:
            self._state.zero_()

    _on_start = _on_stop = _reset_state = _rewind

    def _scan(self, rate_buf: DeviceBuffer, duration: int):
        """positions and their (min, max) for a rate stream; advances the device head."""
        if self._state is None:
            self._state = DeviceBuffer((1,), np.float64, zero=True)
            self._range_dev = DeviceBuffer((2,), np.float64)
            self._workspace = DeviceBuffer((_WORKSPACE_DOUBLES,), np.float64)
        if self._positions is None or self._positions.shape[0] < duration:
            self._positions = DeviceBuffer((duration,), np.float64)
        check(lib().pgx_timewarp_scan(self._positions.ptr, self._range_dev.ptr, self._state.ptr, self._workspace.ptr,
                                      rate_buf.ptr, duration), "pgx_timewarp_scan")
        lo, hi = (float(v) for v in self._range_dev.to_host())
        self.d2h_reads += 1
        return self._positions, lo, hi

    def _render(self, start: int, duration: int) -> Snippet:
        cubic = getattr(self._interpolation, "value", self._interpolation) == "cubic"
        positions, pos0, rate, guard = None, 0.0, 0.0, 0
        if self._rate_is_pe:
            _, rate_buf = self._control_stream(self._rate, start, duration)
            positions, lo, hi = self._scan(rate_buf, duration)
        elif not NO_READBACK:
            if self._const_rate is None or self._const_rate.shape[0] < duration:
                self._const_rate = DeviceBuffer.from_host(np.full((duration, 1), float(self._rate), np.float32))
            positions, lo, hi = self._scan(self._const_rate, duration)
        else:
            pos0, rate, guard = self._pos, float(self._rate), 1
            last = pos0 + float(duration - 1) * rate                  # the kernel's expression for frame duration - 1
            lo, hi = (min(pos0, last), max(pos0, last)) if last == last else (last, last)     # NaN is not ordered
            self._pos = pos0 + float(duration) * rate
        self._last_render_end = start + duration
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("TimeWarpPE: head position is not finite")
        margin = 2 if cubic else 1
        win_start = int(np.floor(lo)) - (margin - 1) - guard
        win_len = int(np.ceil(hi)) + margin + guard - win_start
        window = self._source.render(win_start, win_len)
        ch = window.channels
        ext = self._source.extent()
        out = new_output(duration, ch)
        check(lib().pgx_timewarp(out.ptr, duration, None if positions is None else positions.ptr, pos0, rate,
                                 window.dev.ptr, win_start, win_len, ch, int(cubic),
                                 int(ext.start is not None), float(ext.start or 0),
                                 int(ext.end is not None), float(ext.end or 0)), "pgx_timewarp")
        return Snippet(start, out)

    def __repr__(self) -> str:
        rate = f"{type(self._rate).__name__}(...)" if self._rate_is_pe else str(self._rate)
        return (f"TimeWarpPE(source={type(self._source).__name__}, rate={rate}, "
                f"interpolation={self._interpolation.value})")
