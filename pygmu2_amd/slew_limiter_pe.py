"""
SlewLimiterPE: the output chases channel 0 of the source at no more than rise_rate / fall_rate units per second
(slew_limiter_pe.py:36-141).  LINEAR clips the step to [-fall_rate / sr, rise_rate / sr]; EXPONENTIAL moves by
min(rate / sr, 1) times the remaining error.

Both are per-sample Python loops in the reference.  One sample's update is a continuous, non-decreasing,
piecewise-linear map of the carried value, so a block is solved time-parallel by Newton rounds over affine pieces
(pgx_slew), as EnvelopePE's attack != release follower is: the samples are literal reference steps from entry levels
within ~1e-13 of the sequential loop's.  The carried value lives in HBM; it is zeroed on start / reset_state() only,
the extent is unbounded, and a render that does not continue the previous one carries the value on.
"""

from __future__ import annotations

from enum import Enum

import numpy as np

from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet

# module switch for measurements: True makes every instance count its Newton rounds on the device (see `stats()`)
COUNT_ROUNDS = False


class SlewMode(Enum):
    LINEAR = "linear"
    EXPONENTIAL = "exponential"


class SlewLimiterPE(ProcessingElement):
    _PASSES_BLOCKS = True              # look_ahead.py: the source is pulled with the caller's (start, duration)
    _LOOK_AHEAD_SAFE = True
    _STATE_FIELDS = ("_state",)

    def __init__(self, source: ProcessingElement, rise_rate: float, fall_rate: float | None = None,
                 mode: SlewMode = SlewMode.LINEAR):
        if rise_rate <= 0:
            raise ValueError("rise_rate must be > 0")
        self._source = source
        self._rise_rate = float(rise_rate)
        self._fall_rate = float(fall_rate) if fall_rate is not None else self._rise_rate
        if self._fall_rate <= 0:
            raise ValueError("fall_rate must be > 0")
        self._mode = mode
        self._state: DeviceBuffer | None = None           # {current}
        self._scratch: DeviceBuffer | None = None
        self._scratch_for = -1
        self._stats: DeviceBuffer | None = None

    source = property(lambda self: self._source)
    rise_rate = property(lambda self: self._rise_rate)
    fall_rate = property(lambda self: self._fall_rate)
    mode = property(lambda self: self._mode)

    def inputs(self) -> list[ProcessingElement]:
        return [self._source]

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int:
        return 1

    def _compute_extent(self) -> Extent:
        return Extent(None, None)

    def _reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    _on_start = _reset_state

    def stats(self) -> dict:
        """Newton round counts since the last call (COUNT_ROUNDS): one 16-byte read."""
        if self._stats is None:
            return {"inner_rounds": 0, "windows": 0, "outer_rounds": 0, "fallbacks": 0}
        inner, windows, outer, fallbacks = (int(v) for v in self._stats.to_host())
        self._stats.zero_()
        return {"inner_rounds": inner, "windows": windows, "outer_rounds": outer, "fallbacks": fallbacks}

    def _render(self, start: int, duration: int) -> Snippet:
        src = self._source.render(start, duration)
        sr = float(self.sample_rate)
        up = self._rise_rate / sr                             # slew_limiter_pe.py:107-111
        down = self._fall_rate / sr
        exponential = getattr(self._mode, "value", self._mode) == "exponential"
        if exponential:
            up, down = min(up, 1.0), min(down, 1.0)
        if self._state is None:
            self._state = DeviceBuffer((1,), np.float64, zero=True)
        if self._scratch_for != duration:
            need = lib().pgx_slew_scratch_bytes(duration)
            if self._scratch is None or self._scratch.nbytes < need:
                self._scratch = DeviceBuffer((need // 8,), np.float64)
            self._scratch_for = duration
        if COUNT_ROUNDS and self._stats is None:
            self._stats = DeviceBuffer((4,), np.int32, zero=True)
        out = new_output(duration, 1)
        check(lib().pgx_slew(out.ptr, src.dev.ptr, src.channels, duration, int(exponential), up, down,
                             self._state.ptr, self._scratch.ptr, None if self._stats is None else self._stats.ptr),
              "pgx_slew")
        return Snippet(start, out)

    def __repr__(self) -> str:
        return (f"SlewLimiterPE(rise_rate={self._rise_rate}, fall_rate={self._fall_rate}, "
                f"mode={self._mode.value})")
