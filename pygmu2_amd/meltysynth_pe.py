"""
MeltysynthPE: SoundFont (.sf2) synthesis as a stereo source (meltysynth_pe.py:28-107).  `.synthesizer` is the object a
MIDI callback drives (note_on, note_off, process_midi_message ...); None until the PE is started.

Two planes.  The control plane (soundfont/synth.py) runs on the host once per block per voice and emits a render table;
the audio plane -- oscillator gather, biquad, ramped stereo mix -- is pgx_soundfont_render (csrc/pgx_soundfont.hip), two
launches per call whatever the number of voices and blocks.  The file's int16 samples are uploaded once at start.

_render(start, duration) ignores `start`, as the reference does: the stream is contiguous.  It serves what the last
block left over (the carry) first, advances ceil((duration - carry) / block_size) blocks, and keeps the new remainder.
An event between two renders is therefore heard from the next block boundary of the synthesizer's own grid on, exactly
as the reference's _block_read arranges it.  Long renders are cut into chunks of at most MAX_CHUNK_ROWS table rows (whole
blocks), one entry call each, so that the scratch (rows * block_size float64) stays bounded.

Not pure, and neither read-ahead nor look-ahead safe: a window rendered ahead would freeze the events for its whole
length, so a graph above this PE renders block by block.
"""

from __future__ import annotations

import os

import numpy as np

from . import device as _dev
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .snippet import Snippet
from .soundfont import SoundFont, Synthesizer
from .source_pe import SourcePE

MAX_CHUNK_ROWS = 4096          # table rows per entry call: 2 MiB of scratch at block_size 64
ICOLS, DCOLS = _dev._ABI.constant("PGX_SOUNDFONT_ICOLS"), _dev._ABI.constant("PGX_SOUNDFONT_DCOLS")


def chunk_blocks(block_rows: np.ndarray, max_rows: int):
    """Cut blocks [0, n) into runs [first, last) of at most max_rows rows each (a single block may exceed it)."""
    n, first, out = len(block_rows) - 1, 0, []
    while first < n:
        last = first + 1
        while last < n and block_rows[last + 1] - block_rows[first] <= max_rows:
            last += 1
        out.append((first, last))
        first = last
    return out


class MeltysynthPE(SourcePE):
    maximum_polyphony = 64         # the reference's SynthesizerSettings default; read at start

    def __init__(self, soundfont_path: str, block_size: int = 64, program: int | None = None):
        self._soundfont_path = os.path.realpath(str(soundfont_path))
        self._block_size = block_size
        self._program = program
        self._synthesizer: Synthesizer | None = None
        self.table_log: list | None = None      # a list: every advance()'s (block_rows, rows_i, rows_d) is appended
        self._release()

    def _release(self) -> None:
        self._synthesizer = None
        self._wave = self._filter_state = self._carry = self._scratch = None
        self._carry_pos = self._carry_count = 0

    @property
    def synthesizer(self) -> Synthesizer | None:
        return self._synthesizer

    def _on_start(self) -> None:
        if not os.path.exists(self._soundfont_path):
            raise FileNotFoundError(f"SoundFont not found: {self._soundfont_path}")
        sound_font = SoundFont.from_file(self._soundfont_path)
        synth = Synthesizer(sound_font, self.sample_rate, self._block_size, self.maximum_polyphony)
        wave = sound_font.wave if len(sound_font.wave) else np.zeros(1, dtype=np.int16)
        self._wave = DeviceBuffer.from_host(wave)
        self._wave_len = len(sound_font.wave)
        self._filter_state = DeviceBuffer((synth.maximum_polyphony, 4), np.float64, zero=True)
        self._carry = DeviceBuffer((synth.block_size, 2), np.float32, zero=True)
        self._carry_pos = self._carry_count = 0
        if self._program is not None:
            synth.process_midi_message(0, 0xC0, self._program, 0)
        self._synthesizer = synth

    def _on_stop(self) -> None:
        self._release()

    def _render(self, start: int, duration: int) -> Snippet:
        synth = self._synthesizer
        if synth is None or duration <= 0:
            return Snippet.from_zeros(start, max(duration, 0), 2)
        L, bs = lib(), synth.block_size
        out = new_output(duration, 2)
        if synth.take_reset():                   # reset() drops what is left of the block being served
            self._carry_count = 0
        served = min(self._carry_count, duration)
        if served:
            check(L.pgx_memcpy_d2d(out.ptr, self._carry.offset_ptr(2 * self._carry_pos), served * 8), "pgx_memcpy_d2d")
            self._carry_pos += served
            self._carry_count -= served
        need = duration - served
        if need == 0:
            return Snippet(start, out)
        n_blocks = -(-need // bs)
        block_rows, rows_i, rows_d = synth.advance(n_blocks)
        if self.table_log is not None:
            self.table_log.append((block_rows, rows_i, rows_d))
        done = served
        for first, last in chunk_blocks(block_rows, MAX_CHUNK_ROWS):
            r0, r1 = int(block_rows[first]), int(block_rows[last])
            frames = min((last - first) * bs, duration - done)
            self._play(L, out.offset_ptr(2 * done), frames, block_rows[first:last + 1] - r0, rows_i[r0:r1],
                       rows_d[r0:r1], bs)
            done += frames
        self._carry_pos, self._carry_count = 0, n_blocks * bs - need
        return Snippet(start, out)

    def _play(self, L, out_ptr, frames, block_rows, rows_i, rows_d, bs) -> None:
        """One entry call: the chunk's table in one upload (float64 rows, int32 rows, offsets), then the two launches."""
        n_rows, n_blocks = len(rows_i), len(block_rows) - 1
        d_bytes, i_bytes = n_rows * DCOLS * 8, n_rows * ICOLS * 4
        packed = np.empty(d_bytes + i_bytes + 4 * (n_blocks + 1), dtype=np.uint8)
        packed[:d_bytes] = np.ascontiguousarray(rows_d, dtype=np.float64).view(np.uint8).reshape(-1)
        packed[d_bytes:d_bytes + i_bytes] = np.ascontiguousarray(rows_i, dtype=np.int32).view(np.uint8).reshape(-1)
        packed[d_bytes + i_bytes:] = np.ascontiguousarray(block_rows, dtype=np.int32).view(np.uint8)
        table = DeviceBuffer.from_host(packed)
        need = max(n_rows, 1) * bs                       # scratch: n_rows * block_size float64, at least one
        if self._scratch is None or self._scratch.shape[0] < need:
            self._scratch = DeviceBuffer((need,), np.float64)
        check(L.pgx_soundfont_render(out_ptr, frames, self._carry.ptr, self._wave.ptr, self._wave_len,
                                     table.ptr + d_bytes + i_bytes, table.ptr + d_bytes, table.ptr, n_rows, n_blocks,
                                     bs, self._filter_state.ptr, self._synthesizer.maximum_polyphony,
                                     self._scratch.ptr), "pgx_soundfont_render")

    def _compute_extent(self) -> Extent:
        return Extent(None, None)

    def channel_count(self) -> int:
        return 2

    def is_pure(self) -> bool:
        return False

    def __repr__(self) -> str:
        prog = f", program={self._program}" if self._program is not None else ""
        return f"MeltysynthPE(soundfont_path={self._soundfont_path!r}, block_size={self._block_size}{prog})"
