"""
ReversePitchEchoPE: pitch-shifted reverse echo (reverse_pitch_echo_pe.py, the arithmetic of
_reverse_pitch_echo_numba).  The input goes through a two-head time-domain pitch shifter into the current echo block;
meanwhile the previous echo block is played back reversed, or alternately forward, under a Hann window, and that
playback -- wet only -- is the output, fed back into the block being written.

Everything carried between renders lives on the device: one record (smoothed block size, read position, indices,
block lengths, direction, buffer parities), the two (rows, C) float64 echo buffers and the pitch history.  A render is
three launches of csrc/pgx_reverse_echo.hip -- plan, pitch, echo -- and copies nothing to the host.

Not `_LOOK_AHEAD_SAFE`: a look-ahead snapshot would copy both echo buffers (2 * rows * C * 8 bytes) per window, so a
sub-graph that contains this PE renders block by block.
"""

from __future__ import annotations

import numpy as np

from . import device as _dev
from ._kernels import DeviceBuffer, check, lib, new_output, ptr
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet


class ReversePitchEchoPE(ProcessingElement):
    _MAX_DELAY_SECONDS = 10.0
    _MIN_BLOCK_SAMPLES = _dev.REVERSE_ECHO_MIN_BLOCK
    _MAX_FEEDBACK = _dev.REVERSE_ECHO_MAX_FEEDBACK

    def __init__(self, source: ProcessingElement, block_seconds=0.25, pitch_ratio=1.0, feedback=0.85,
                 alternate_direction=0.0, smoothing_samples: int = 2400):
        self._source = source
        self._block_seconds = block_seconds
        self._pitch_ratio = pitch_ratio
        self._feedback = feedback
        self._alternate_direction = alternate_direction
        self._smoothing_samples = max(1, int(smoothing_samples))
        self._block_is_pe = isinstance(block_seconds, ProcessingElement)
        self._pitch_is_pe = isinstance(pitch_ratio, ProcessingElement)
        self._fb_is_pe = isinstance(feedback, ProcessingElement)
        self._alt_is_pe = isinstance(alternate_direction, ProcessingElement)
        self._state: DeviceBuffer | None = None      # one device.REVERSE_ECHO_STATE record
        self._echo: DeviceBuffer | None = None       # (2, rows, C) float64: buffer A, buffer B
        self._pitch: DeviceBuffer | None = None      # (2, pitch_len, C) float64: the history in time order, two halves
        self._ws: DeviceBuffer | None = None

    @property
    def source(self) -> ProcessingElement:
        return self._source

    def inputs(self) -> list[ProcessingElement]:
        out = [self._source]
        for is_pe, param in ((self._block_is_pe, self._block_seconds), (self._pitch_is_pe, self._pitch_ratio),
                             (self._fb_is_pe, self._feedback), (self._alt_is_pe, self._alternate_direction)):
            if is_pe:
                out.append(param)
        return out

    def is_pure(self) -> bool:
        return False

    def channel_count(self) -> int | None:
        return self._source.channel_count()

    def _compute_extent(self) -> Extent:
        ext = self._source.extent()
        for param in self.inputs()[1:]:
            ext = ext.intersection(param.extent()) or ext
        return ext

    # ------------------------------------------------------------------ sizes (reverse_pitch_echo_pe.py:478-514)
    def _buffer_rows(self) -> int:
        return max(self._MIN_BLOCK_SAMPLES + 1, int(self._MAX_DELAY_SECONDS * self.sample_rate))

    def _pitch_len(self) -> int:
        return max(2, int(self.sample_rate / 60))

    def _clamp_block_samples(self, samples: float) -> int:
        if not np.isfinite(samples):
            return self._MIN_BLOCK_SAMPLES
        max_samples = int(self._MAX_DELAY_SECONDS * self.sample_rate) - 1
        return int(np.round(np.clip(samples, self._MIN_BLOCK_SAMPLES, max_samples)))

    def _initial_smoothed(self) -> int:
        seconds = 0.25 if self._block_is_pe else float(self._block_seconds)
        return self._clamp_block_samples(seconds * self.sample_rate)

    # ------------------------------------------------------------------ lifecycle
    def _allocate(self, channels: int) -> None:
        self._echo = DeviceBuffer((2, self._buffer_rows(), channels), np.float64, zero=True)
        self._pitch = DeviceBuffer((2, self._pitch_len(), channels), np.float64, zero=True)
        rec = np.zeros(1, dtype=_dev.REVERSE_ECHO_STATE)
        smoothed = self._initial_smoothed()
        rec["smoothed"] = float(smoothed)
        rec["current_block"] = smoothed
        rec["reverse"] = 1
        rec["current_is_a"] = 1
        self._state = _dev.upload_structs(rec)

    def _on_start(self) -> None:
        self._allocate(self._source.channel_count() or 1)

    def _on_stop(self) -> None:
        self._state = None
        self._echo = None
        self._pitch = None

    # no _reset_state: the reference has none, reset_state() changes nothing

    def _render(self, start: int, duration: int) -> Snippet:
        src = self._source.render(start, duration)
        ch = src.channels
        if self._echo is None or self._pitch is None or self._state is None or self._echo.shape[2] != ch:
            self._allocate(ch)
        block_s, block_buf = self._control_stream(self._block_seconds, start, duration)
        pitch_s, pitch_buf = self._control_stream(self._pitch_ratio, start, duration)
        fb_s, fb_buf = self._control_stream(self._feedback, start, duration)
        alt_s, alt_buf = self._control_stream(self._alternate_direction, start, duration)
        L = lib()
        need = L.pgx_reverse_echo_workspace_bytes(duration, ch)
        if self._ws is None or self._ws.nbytes < need:
            self._ws = DeviceBuffer((need,), np.uint8)
        rows, plen = self._echo.shape[1], self._pitch.shape[1]
        out = new_output(duration, ch)
        check(L.pgx_reverse_echo(out.ptr, src.dev.ptr, duration, ch, float(self.sample_rate),
                                 block_s or 0.0, ptr(block_buf), pitch_s or 0.0, ptr(pitch_buf), fb_s or 0.0, ptr(fb_buf),
                                 alt_s or 0.0, ptr(alt_buf), self._smoothing_samples, self._state.ptr, self._echo.ptr,
                                 self._echo.offset_ptr(rows * ch), rows, self._pitch.ptr, plen, self._ws.ptr),
              "pgx_reverse_echo")
        return Snippet(start, out)

    def __repr__(self) -> str:
        def show(is_pe, param):
            return f"{param.__class__.__name__}(...)" if is_pe else param
        return (f"ReversePitchEchoPE(source={self._source.__class__.__name__}, "
                f"block_seconds={show(self._block_is_pe, self._block_seconds)}, "
                f"pitch_ratio={show(self._pitch_is_pe, self._pitch_ratio)}, "
                f"feedback={show(self._fb_is_pe, self._feedback)})")
