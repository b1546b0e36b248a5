"""
TrackHoldPE: follow the source while the gate is open (gate > 0.5), freeze the last tracked value while it is
closed (track_hold_pe.py:21-92).  The scan and the state are SampleHoldPE's (sample_hold_pe.py, pgx_hold); only
the threshold differs.
"""

from __future__ import annotations

from .processing_element import ProcessingElement
from .sample_hold_pe import _HoldPE


class TrackHoldPE(_HoldPE):
    _THRESHOLD = 0.5
    _CONTROL_NAME = "gate"

    def __init__(self, source: ProcessingElement, gate: ProcessingElement, initial_value: float = 0.0):
        super().__init__(source, gate, initial_value)

    gate = property(lambda self: self._control)
