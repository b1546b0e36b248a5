"""
FunctionGenPE: naive function generator without anti-aliasing (function_gen_pe.py:36-209): a +-1 rectangle
(phase < duty), or a saw <-> triangle morph by duty (0: rising saw, 0.5: triangle, 1: falling saw).  Frequency, duty
and phase are scalars or PEs.

All scalars -> pure: phase = mod(mod(n * (f / sr), 1) + phase, 1) from the frame index, one launch
(pgx_function_gen_pure), bit-exact.  Any PE parameter -> the phase is the running sum of f / sr, carried across
contiguous renders in HBM and restarted from 0 on a seek, on start and on stop; the sum is a float64 prefix scan
over workgroup segments (pgx_function_gen_stateful), so a sample may differ from the reference's sequential
np.cumsum by the re-association of that sum (~1e-13 cycle) unless the sums are exact in float64.
"""

from __future__ import annotations

import numpy as np

from . import device
from ._kernels import DeviceBuffer, check, lib, new_output
from .config import get_sample_rate
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet

_WORKSPACE_DOUBLES = device.CONTROL_WORKSPACE_DOUBLES


class FunctionGenPE(ProcessingElement):
    WAVE_RECTANGLE = "rectangle"
    WAVE_SAWTOOTH = "sawtooth"

    _PASSES_BLOCKS = True
    _READ_AHEAD_SAFE = True            # all scalars: a function of the frame index
    _LOOK_AHEAD_SAFE = True            # PE-driven parameters: carried phase
    _STATE_FIELDS = ("_state", "_last_render_end")

    def __init__(self, frequency=1.0, duty_cycle=0.5, phase=0.0, waveform: str = "rectangle", channels: int = 1):
        self._frequency = frequency
        self._duty_cycle = duty_cycle
        self._phase_in = phase
        self._waveform = str(waveform).lower()
        self._channels = int(channels)
        if self._waveform not in (self.WAVE_RECTANGLE, self.WAVE_SAWTOOTH):
            raise ValueError(f"waveform must be 'rectangle' or 'sawtooth', got {waveform!r}")
        if self._channels < 1:
            raise ValueError(f"channels must be >= 1, got {channels}")
        self._state: DeviceBuffer | None = None           # stateful path: carried phase in cycles
        self._workspace: DeviceBuffer | None = None
        self._last_render_end: int | None = None

    frequency = property(lambda self: self._frequency)
    duty_cycle = property(lambda self: self._duty_cycle)
    phase = property(lambda self: self._phase_in)
    waveform = property(lambda self: self._waveform)

    def inputs(self) -> list[ProcessingElement]:
        return [p for p in (self._frequency, self._duty_cycle, self._phase_in) if isinstance(p, ProcessingElement)]

    def is_pure(self) -> bool:
        return not self.inputs()

    def channel_count(self) -> int:
        return self._channels

    def _compute_extent(self) -> Extent:
        ext = Extent(None, None)
        for p in self.inputs():
            ext = ext.intersection(p.extent())
        return ext

    def _reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()
        self._last_render_end = None

    _on_start = _reset_state
    _on_stop = _reset_state

    def _render(self, start: int, duration: int) -> Snippet:
        saw = int(self._waveform == self.WAVE_SAWTOOTH)
        sr = float(get_sample_rate())
        out = new_output(duration, self._channels)
        if self.is_pure():
            dt = float(np.float64(self._frequency) / sr)                      # freq / sr (:164)
            check(lib().pgx_function_gen_pure(out.ptr, start, duration, self._channels, saw, dt,
                                              float(self._phase_in), float(self._duty_cycle)),
                  "pgx_function_gen_pure")
            return Snippet(start, out)
        if self._state is None:
            self._state = DeviceBuffer((1,), np.float64, zero=True)
            self._workspace = DeviceBuffer((_WORKSPACE_DOUBLES,), np.float64)
        if self._last_render_end is None or start != self._last_render_end:
            self._state.zero_()
        f_s, f_buf = self._control_stream(self._frequency, start, duration)
        d_s, d_buf = self._control_stream(self._duty_cycle, start, duration)
        p_s, p_buf = self._control_stream(self._phase_in, start, duration)
        check(lib().pgx_function_gen_stateful(
            out.ptr, duration, self._channels, saw, sr, 0.0 if f_s is None else f_s, 0.0 if d_s is None else d_s,
            0.0 if p_s is None else p_s, None if f_buf is None else f_buf.ptr, None if d_buf is None else d_buf.ptr,
            None if p_buf is None else p_buf.ptr, self._state.ptr, self._workspace.ptr), "pgx_function_gen_stateful")
        self._last_render_end = start + duration
        return Snippet(start, out)

    def __repr__(self) -> str:
        freq = type(self._frequency).__name__ if isinstance(self._frequency, ProcessingElement) else str(self._frequency)
        duty = type(self._duty_cycle).__name__ if isinstance(self._duty_cycle, ProcessingElement) else str(self._duty_cycle)
        return (f"FunctionGenPE(frequency={freq}, duty_cycle={duty}, "
                f"waveform={self._waveform!r}, channels={self._channels})")
