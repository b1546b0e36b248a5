"""
ControlPE: a constant that another thread can move while a stream runs (control_pe.py:28-79).  set_value(v) puts v on
a queue from any thread; a render drains the queue, keeps the last value and fills its block with it (pgx_fill).

Not pure, and neither read-ahead nor look-ahead safe: a window rendered ahead would freeze the control for its whole
length.  A graph above a ControlPE therefore renders block by block, and a new value is heard from the next render on.
"""

from __future__ import annotations

import queue

from ._kernels import check, lib, new_output
from .snippet import Snippet
from .source_pe import SourcePE


class ControlPE(SourcePE):
    def __init__(self, initial_value: float = 0.0, channels: int = 1):
        self._value = initial_value
        self._channels = channels
        self._queue: queue.Queue = queue.Queue()

    def set_value(self, value: float) -> None:
        """Thread-safe: hand over a new value from any thread."""
        self._queue.put_nowait(value)

    @property
    def value(self) -> float:
        """The last value a render consumed."""
        return self._value

    def _render(self, start: int, duration: int) -> Snippet:
        try:
            while True:
                self._value = self._queue.get_nowait()
        except queue.Empty:
            pass
        out = new_output(duration, self._channels)
        # np.full(..., value, dtype=float32): the value is rounded to float32 once
        check(lib().pgx_fill(out.ptr, duration * self._channels, float(self._value)), "pgx_fill")
        return Snippet(start, out)

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int:
        return self._channels

    def __repr__(self) -> str:
        return f"ControlPE(value={self._value}, channels={self._channels})"
