"""
SampleHoldPE: latch the source on every trigger sample (trigger > 0), hold the value in between
(sample_hold_pe.py:21-92).  TrackHoldPE (track_hold_pe.py) is the same scan with the threshold 0.5.

The reference walks the block sample by sample.  Here out[i] = source[j], j the last frame <= i whose control sample
passes -- a max-scan over frame indices and a gather (pgx_hold), bit-exact however the stream is cut.  The held
value lives in HBM as one double: the float64 `initial_value` until the first latch, a float32 sample afterwards.
Only channel 0 of source and control is read, in place.  The extent is unbounded whatever the inputs' extents are,
the state goes back to `initial_value` on start / reset_state() only, and a render that does not continue the
previous one carries the held value on.
"""

from __future__ import annotations

import numpy as np

from . import device
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet

_WORKSPACE_DOUBLES = device.CONTROL_WORKSPACE_DOUBLES


class _HoldPE(ProcessingElement):
    _PASSES_BLOCKS = True              # look_ahead.py: inputs are pulled with the caller's (start, duration)
    _LOOK_AHEAD_SAFE = True
    _STATE_FIELDS = ("_state",)
    _THRESHOLD = 0.0
    _CONTROL_NAME = "trigger"

    def __init__(self, source: ProcessingElement, control: ProcessingElement, initial_value: float = 0.0):
        self._source = source
        self._control = control
        self._initial_value = float(initial_value)
        self._state: DeviceBuffer | None = None           # {held}; None: still the initial value
        self._workspace: DeviceBuffer | None = None

    source = property(lambda self: self._source)
    initial_value = property(lambda self: self._initial_value)

    def inputs(self) -> list[ProcessingElement]:
        return [self._source, self._control]

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int:
        return 1

    def _compute_extent(self) -> Extent:
        return Extent(None, None)

    def _reset_state(self) -> None:
        self._state = None

    _on_start = _reset_state

    def _render(self, start: int, duration: int) -> Snippet:
        control = self._control.render(start, duration)       # the reference pulls the control first
        src = self._source.render(start, duration)
        if self._state is None:
            self._state = DeviceBuffer.from_host(np.array([self._initial_value], dtype=np.float64))
        if self._workspace is None:
            self._workspace = DeviceBuffer((_WORKSPACE_DOUBLES,), np.float64)
        out = new_output(duration, 1)
        check(lib().pgx_hold(out.ptr, src.dev.ptr, src.channels, control.dev.ptr, control.channels, duration,
                             self._THRESHOLD, self._state.ptr, self._workspace.ptr), "pgx_hold")
        return Snippet(start, out)

    def __repr__(self) -> str:
        return (f"{type(self).__name__}(source={type(self._source).__name__}, "
                f"{self._CONTROL_NAME}={type(self._control).__name__}, initial_value={self._initial_value})")


class SampleHoldPE(_HoldPE):
    def __init__(self, source: ProcessingElement, trigger: ProcessingElement, initial_value: float = 0.0):
        super().__init__(source, trigger, initial_value)

    trigger = property(lambda self: self._control)
