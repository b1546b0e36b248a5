"""SlicePE: cut [start, start+duration) out of a source, shift it to time 0 and optionally taper its edges
(slice_pe.py:32-132).  Composed as the reference composes it -- CropPE -> DelayPE(-start) -> GainPE(gain=ArrayPE(env)) --
with the envelope built in float32 by the reference's expressions, so no kernel of its own."""

from __future__ import annotations

import numpy as np

from .array_pe import ArrayPE
from .crop_pe import CropPE
from .delay_pe import DelayPE
from .extent import Extent
from .gain_pe import GainPE
from .processing_element import ProcessingElement


class SlicePE(ProcessingElement):
    _PASSES_BLOCKS = True              # look_ahead.py: the composed graph is pulled with the caller's (start, duration)
    _READ_AHEAD_SAFE = True

    def __init__(self, source: ProcessingElement, start: int, duration: int, *,
                 fade_in_seconds: float | None = None, fade_out_seconds: float | None = None):
        self._source = source
        self._start = int(start)
        self._duration = int(duration)
        self._fade_in_seconds = fade_in_seconds
        self._fade_out_seconds = fade_out_seconds
        if self._duration < 0:
            raise ValueError(f"duration must be >= 0, got {duration}")
        crop = CropPE(self._source, self._start, self._duration)
        self._base = DelayPE(crop, delay=-self._start)
        self._fade_in = int(round(fade_in_seconds * self.sample_rate)) if fade_in_seconds is not None else 0
        self._fade_out = int(round(fade_out_seconds * self.sample_rate)) if fade_out_seconds is not None else 0
        if self._duration > 0 and (self._fade_in > 0 or self._fade_out > 0):
            env = np.ones((self._duration,), dtype=np.float32)
            fi = min(self._fade_in, self._duration)
            fo = min(self._fade_out, self._duration)
            if fi > 0:
                ramp = (np.arange(fi, dtype=np.float32) + 1.0) / float(fi)
                env[:fi] = np.minimum(env[:fi], ramp)
            if fo > 0:
                ramp = 1.0 - (np.arange(fo, dtype=np.float32) + 1.0) / float(fo)
                env[-fo:] = np.minimum(env[-fo:], ramp)
            self._out = GainPE(self._base, gain=ArrayPE(env))
        else:
            self._out = self._base

    source = property(lambda self: self._source)
    start = property(lambda self: self._start)
    duration = property(lambda self: self._duration)
    fade_in_samples = property(lambda self: self._fade_in)
    fade_out_samples = property(lambda self: self._fade_out)

    def inputs(self) -> list[ProcessingElement]:
        return [self._out]             # the composed graph, so that lifecycle calls reach its PEs

    def is_pure(self) -> bool:
        return self._out.is_pure()

    def channel_count(self) -> int | None:
        return self._out.channel_count()

    def _compute_extent(self) -> Extent:
        return self._out.extent()

    def _render(self, start: int, duration: int):
        return self._out.render(start, duration)

    def __repr__(self) -> str:
        return (f"SlicePE(source={self._source.__class__.__name__}, start={self._start}, duration={self._duration}, "
                f"fade_in_seconds={self._fade_in_seconds}, fade_out_seconds={self._fade_out_seconds})")
