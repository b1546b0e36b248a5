"""
TransformPE: apply an element-wise function to a source (transform_pe.py:19-152).

`func` is a descriptor from pygmu2_amd.transforms (or np.abs / np.tanh / np.sqrt /
np.square, which are recognised): the whole chain runs in one device kernel in float64
and rounds to float32 once, like the reference's  func(data.astype(float64)).astype(float32).
pitch_to_freq / freq_to_pitch / semitones_to_ratio / ratio_to_semitones of conversions.py (themselves, a
functools.partial with keywords, or transforms.PitchToFreq ...) are such descriptors: a chain that holds one runs in
pgx_tuning, every other chain in pgx_transform as before.  A tuning step with a None follows temperament.py's globals:
they are read when a block is rendered, so such a TransformPE takes no part in read-ahead (a window rendered ahead
would hold the old tuning's samples after set_temperament); one with everything explicit does.

Any other callable is the user's own host code.  It is honoured the way the reference
does it, on a host copy of the block (device -> host -> func -> device), with the
reference's shape repair (transform_pe.py:136-147); that crossing is the callable's cost,
not a fallback of this library.
"""

from __future__ import annotations

from typing import Callable

import numpy as np

from . import device as _dev
from . import temperament as _tm
from . import transforms as _tf
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet


class TransformPE(ProcessingElement):
    _PASSES_BLOCKS = True              # look_ahead.py: inputs are pulled with the caller's (duration)
    _READ_AHEAD_SAFE = True            # named element-wise chains only (see the condition)

    def _read_ahead_condition(self) -> bool:
        return self._lowered is not None and not self._follows_globals

    def __init__(self, source: ProcessingElement, func: Callable[[np.ndarray], np.ndarray],
                 name: str | None = None):
        self._source = source
        self._func = func
        self._name = name or getattr(func, "__name__", "transform")
        self._lowered = _tf.lower(func)
        self._follows_globals = self._lowered is not None and self._lowered.follows_globals()
        self._ops_dev: DeviceBuffer | None = None
        self._nops = 0
        self._tuning_dev: tuple[DeviceBuffer, DeviceBuffer] | None = None     # (records, tables) of pgx_tuning
        self._epoch = -1               # temperament.epoch() the uploaded program was resolved at
        self._on_host = False          # the globals resolved to host code (a CustomTemperament)

    source = property(lambda self: self._source)
    func = property(lambda self: self._func)
    name = property(lambda self: self._name)

    def inputs(self) -> list[ProcessingElement]:
        return [self._source]

    def is_pure(self) -> bool:
        return True

    def channel_count(self) -> int | None:
        return self._source.channel_count()

    def _compute_extent(self) -> Extent:
        return self._source.extent()

    def _render(self, start: int, duration: int) -> Snippet:
        src = self._source.render(start, duration)
        if self._lowered is None:
            return self._render_host_callable(start, src)
        if self._ops_dev is None or (self._follows_globals and self._epoch != _tm.epoch()):
            self._upload_program()
        if self._on_host:
            return self._render_host_callable(start, src)
        out = new_output(duration, src.channels)
        if self._tuning_dev is not None:
            records, tables = self._tuning_dev
            check(lib().pgx_tuning(out.ptr, src.dev.ptr, duration * src.channels, self._ops_dev.ptr, self._nops,
                                   records.ptr, tables.ptr), "pgx_tuning")
            return Snippet(start, out)
        check(lib().pgx_transform(out.ptr, src.dev.ptr, duration * src.channels, self._ops_dev.ptr,
                                  self._nops), "pgx_transform")
        return Snippet(start, out)

    def _upload_program(self) -> None:
        """The chain's ops as device tables: pgx_transform_op, or -- with a tuning step -- pgx_tuning_op plus one
        pgx_tuning_record per step and the just tables they point into."""
        self._epoch = _tm.epoch()
        try:
            ops = self._lowered.ops()
        except LookupError:            # the global temperament is host code now
            self._on_host, self._ops_dev = True, None
            return
        self._on_host = False
        tuned = [op for op in ops if op[0] in _tf.TUNING_CODES]
        if not tuned:
            table = np.zeros(max(len(ops), 1), dtype=_dev.TRANSFORM_OP)
            for i, (code, p0, p1) in enumerate(ops):
                table[i] = (code, 0, p0, p1)
            self._tuning_dev = None
        else:
            table = np.zeros(len(ops), dtype=_dev.TUNING_OP)
            records = np.zeros(len(tuned), dtype=_dev.TUNING_RECORD)
            tables, at = [np.zeros(1)], 1                  # never an empty buffer
            for i, (code, p0, p1) in enumerate(ops):
                if code not in _tf.TUNING_CODES:
                    table[i] = (code, 0, p0, p1)
                    continue
                k = sum(1 for op in ops[:i] if op[0] in _tf.TUNING_CODES)
                table[i] = (code, k, 0.0, 0.0)
                notes = 0
                if p0.just:
                    notes = (len(p0.table) - 1) // 2
                    tables.append(np.asarray(p0.table, dtype=np.float64))
                records[k] = (p0.reference_pitch, p0.reference_freq, p0.divisions, at if p0.just else 0, notes, 0)
                at += len(p0.table) if p0.just else 0
            self._tuning_dev = (DeviceBuffer.from_host(records.view(np.uint8)),
                                DeviceBuffer.from_host(np.concatenate(tables)))
        self._ops_dev = DeviceBuffer.from_host(table.view(np.uint8))
        self._nops = len(ops)

    def _render_host_callable(self, start: int, src: Snippet) -> Snippet:
        data = src.data.astype(np.float64)
        res = np.asarray(self._func(data))
        if data.ndim == 2 and res.ndim == 1:
            res = res.reshape(-1, data.shape[1])
        elif data.ndim == 2 and res.ndim == 2 and res.shape[1] != data.shape[1]:
            res = np.broadcast_to(res, data.shape) if res.shape[1] == 1 else res[:, :data.shape[1]]
        return Snippet(start, np.ascontiguousarray(res.astype(np.float32)))

    def __repr__(self) -> str:
        return f"TransformPE(source={type(self._source).__name__}, func={self._name})"
