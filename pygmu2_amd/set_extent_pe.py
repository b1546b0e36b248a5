"""SetExtentPE: force a source to [start, start+duration), padding or truncating (set_extent_pe.py:17-77).  Unlike
CropPE the extent is the given one, not its intersection with the source's; either bound may be None (open)."""

from __future__ import annotations

from .extent import ExtendMode, Extent
from .extent_window_pe import _ExtentWindowPE
from .processing_element import ProcessingElement


class SetExtentPE(_ExtentWindowPE):
    def __init__(self, source: ProcessingElement, start: int | None, duration: int | None,
                 extend_mode: ExtendMode = ExtendMode.ZERO):
        if duration is not None and duration < 0:
            raise ValueError(f"duration must be >= 0, got {duration}")
        self._start = int(start) if start is not None else None
        self._duration = int(duration) if duration is not None else None
        end = None
        if self._duration is not None:
            end = self._duration if self._start is None else self._start + self._duration
        super().__init__(source, Extent(self._start, end), extend_mode)

    start = property(lambda self: self._start)
    duration = property(lambda self: self._duration)
    end = property(lambda self: self._extent.end)

    def _compute_extent(self) -> Extent:
        return self._extent

    def __repr__(self) -> str:
        start = str(self._extent.start) if self._extent.start is not None else "None"
        end = str(self._extent.end) if self._extent.end is not None else "None"
        ext = f", extend_mode={self._extend_mode.value}" if self._extend_mode != ExtendMode.ZERO else ""
        return f"SetExtentPE(source={type(self._source).__name__}, extent=Extent({start}, {end}){ext})"
