"""
AnalogOscPE: polyBLEP rectangle with PWM and a duty-morphed sawtooth / triangle (analog_osc_pe.py:34-267).

float64 on the device, one float32 rounding on output (csrc/pgx_sources.hip).  All-scalar parameters -> pure: the
rectangle is a function of the frame index (pgx_analog_osc_pure, one element-wise launch); the sawtooth integrates
its BLEP-corrected derivative from a start value recomputed at every render, so -- as in the reference -- its samples
depend on how a stream is cut into requests, and it is rendered request by request (no read-ahead, no look-ahead).
Any PE parameter -> stateful: the phase is an exclusive prefix sum of f / sr over the carried phase and the sawtooth
integrates over the carried value, both carried in a device state blob (pgx_analog_osc_stateful); a render that does
not continue the previous one restarts at phase 0 / saw -1.
"""

from __future__ import annotations

import numpy as np

from ._kernels import DeviceBuffer, check, lib, new_output, ptr
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet


class AnalogOscPE(ProcessingElement):
    WAVE_RECTANGLE = "rectangle"
    WAVE_SAWTOOTH = "sawtooth"

    _READ_AHEAD_SAFE = True            # the pure rectangle is a function of the index (see _read_ahead_condition)
    _LOOK_AHEAD_SAFE = True            # the stateful form carries phase and saw value sample by sample
    _STATE_FIELDS = ("_state", "_last_render_end")

    def __init__(self, frequency=440.0, duty_cycle=0.5, waveform: str = "rectangle", channels: int = 1):
        self._frequency = frequency
        self._duty_cycle = duty_cycle
        self._waveform = str(waveform).lower()
        self._channels = int(channels)
        if self._waveform not in (self.WAVE_RECTANGLE, self.WAVE_SAWTOOTH):
            raise ValueError(f"waveform must be 'rectangle' or 'sawtooth', got {waveform!r}")
        if self._channels < 1:
            raise ValueError(f"channels must be >= 1, got {channels}")
        self._state: DeviceBuffer | None = None     # {phase, saw value} of the stateful form
        self._last_render_end: int | None = None
        self._ws: DeviceBuffer | None = None

    frequency = property(lambda self: self._frequency)
    duty_cycle = property(lambda self: self._duty_cycle)
    waveform = property(lambda self: self._waveform)

    def _read_ahead_condition(self) -> bool:
        # a pure sawtooth restarts its integration at every request: a window would change the samples
        return self._waveform == self.WAVE_RECTANGLE

    def _look_ahead_condition(self) -> bool:
        return not (self.is_pure() and self._waveform == self.WAVE_SAWTOOTH)

    def inputs(self) -> list[ProcessingElement]:
        return [p for p in (self._frequency, self._duty_cycle) if isinstance(p, ProcessingElement)]

    def is_pure(self) -> bool:
        return not self.inputs()

    def channel_count(self) -> int:
        return self._channels

    def _on_start(self) -> None:
        self._reset_state()

    def _on_stop(self) -> None:
        self._reset_state()

    def _reset_state(self) -> None:
        self._last_render_end = None       # the next render restarts at phase 0 / saw -1

    def _compute_extent(self) -> Extent:
        result = Extent(None, None)
        for pe_input in self.inputs():
            result = result.intersection(pe_input.extent())
        return result

    def _workspace(self, duration: int):
        need = lib().pgx_analog_osc_workspace_bytes(duration)
        if self._ws is None or self._ws.nbytes < need:
            self._ws = DeviceBuffer((max(need, 1),), np.uint8)
        return self._ws

    def _render(self, start: int, duration: int) -> Snippet:
        out = new_output(duration, self._channels)
        L = lib()
        sr = float(self.sample_rate)
        wave = 0 if self._waveform == self.WAVE_RECTANGLE else 1
        if self.is_pure():
            ws = self._workspace(duration).ptr if wave else None
            check(L.pgx_analog_osc_pure(out.ptr, start, duration, self._channels, sr, wave, float(self._frequency),
                                        float(self._duty_cycle), ws), "pgx_analog_osc_pure")
            return Snippet(start, out)
        f_s, f_buf = self._control_stream(self._frequency, start, duration)
        d_s, d_buf = self._control_stream(self._duty_cycle, start, duration)
        restart = self._last_render_end is None or start != self._last_render_end
        if self._state is None:
            self._state = DeviceBuffer((2,), np.float64, zero=True)
        check(L.pgx_analog_osc_stateful(out.ptr, duration, self._channels, sr, wave,
                                        0.0 if f_s is None else f_s, 0.0 if d_s is None else d_s,
                                        ptr(f_buf), ptr(d_buf), int(restart), self._state.ptr,
                                        self._workspace(duration).ptr), "pgx_analog_osc_stateful")
        self._last_render_end = start + duration
        return Snippet(start, out)

    def __repr__(self) -> str:
        def s(p):
            return p.__class__.__name__ if isinstance(p, ProcessingElement) else str(p)
        return (f"AnalogOscPE(frequency={s(self._frequency)}, duty_cycle={s(self._duty_cycle)}, "
                f"waveform={self._waveform!r}, channels={self._channels})")
