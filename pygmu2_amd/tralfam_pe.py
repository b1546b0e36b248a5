"""
TralfamPE: spread a finite source's spectrum randomly across its time span (tralfam_pe.py:25-148).

The reference renders the whole extent of its source once, takes np.fft.fft per channel, keeps the magnitudes, replaces
every phase by default_rng(seed).random(shape) * 2 pi, inverts, keeps the real part as float32, optionally scales the
peak to `normalize_peak`, caches the (N, C) result and serves slices of it.  Here all of that runs on the device
(pgx_tralfam, csrc/pgx_spectral.hip): a float64 DFT of the whole extent -- any length up to 2^21 frames, Bluestein's
chirp-z where N is not a power of two -- the phases drawn from numpy's PCG64 stream by skip-ahead (draw k*C + c, as
rng.random((N, C)) fills row-major), and the peak reduced and applied without leaving HBM.  The host asks numpy for the
seeded (state, inc) once, exactly as NoisePE does; seed=None draws fresh entropy per instance.

The source is pulled ONCE, for exactly (extent.start, extent.duration), at the first render that lands in a finite
extent -- a NoisePE below consumes the draws the reference consumes.  The cached result lives in HBM; a render inside
the extent hands out its rows, one across an edge is composed by pgx_window_copy.

Windows: a slice of a cached buffer depends on the frame index alone, so the class is _READ_AHEAD_SAFE -- a pure graph
above may render many blocks at once through it (that is one window copy, and still one pull of the source).  Read-ahead
only opens such a window when the source is itself pure and eligible, and _look_ahead_condition holds look-ahead
windows of a stateful graph above to the same rule (as CachePE does): settling a window restores the states below it to
before the one pull and renders the consumed blocks again -- from the cache, so a stateful source (a NoisePE) would be
left as if it had never been pulled.  Over such a source the graph stays block by block, where each block is a row view
or one launch.
"""

from __future__ import annotations

import numpy as np

from . import device as _dev
from . import spectral as _spectral
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .processing_element import ProcessingElement
from .snippet import Snippet

_MASK64 = (1 << 64) - 1


class TralfamPE(ProcessingElement):
    _READ_AHEAD_SAFE = True

    def _look_ahead_condition(self) -> bool:
        from . import read_ahead
        return read_ahead.eligible(self._source)

    def __init__(self, source: ProcessingElement, seed: int | None = None, normalize_peak: float | None = None):
        self._source = source
        self._seed = seed
        if normalize_peak is not None and (normalize_peak <= 0 or not np.isfinite(normalize_peak)):
            raise ValueError(f"normalize_peak must be a positive finite number, got {normalize_peak!r}")
        self._normalize_peak = normalize_peak
        self._mogrified: DeviceBuffer | None = None       # (frames, channels) float32 in HBM

    source = property(lambda self: self._source)
    seed = property(lambda self: self._seed)
    normalize_peak = property(lambda self: self._normalize_peak)

    def inputs(self) -> list[ProcessingElement]:
        return [self._source]

    def _compute_extent(self) -> Extent:
        return self._source.extent()

    def channel_count(self) -> int | None:
        return self._source.channel_count()

    def is_pure(self) -> bool:
        return True

    def _seeded_generator(self) -> DeviceBuffer:
        s = np.random.PCG64(self._seed).state["state"]
        state, inc = int(s["state"]), int(s["inc"])
        rec = np.zeros(1, dtype=_dev.NOISE_PARAMS)
        rec["state_hi"], rec["state_lo"] = state >> 64, state & _MASK64
        rec["inc_hi"], rec["inc_lo"] = inc >> 64, inc & _MASK64
        return _dev.upload_structs(rec)

    def _mogrify(self) -> DeviceBuffer:
        """Render the whole source, DFT -> random phases -> inverse DFT; cache and return the (frames, channels) result."""
        if self._mogrified is not None:
            return self._mogrified
        ext = self.extent()
        if ext.start is None or ext.end is None:
            raise ValueError(f"{self.__class__.__name__} requires finite source extent; "
                             f"got start={ext.start}, end={ext.end}")
        n = ext.duration
        if n is None or n <= 0:
            raise ValueError(f"{self.__class__.__name__} requires positive extent duration; got duration={n}")
        _spectral.check_length(n, self.__class__.__name__)
        snippet = self._source.render(ext.start, n)
        channels = snippet.channels
        plan = _spectral.plan_for(n)
        need = lib().pgx_tralfam_workspace_bytes(n, channels)
        if not need:
            raise ValueError(f"{self.__class__.__name__}: unsupported shape ({n}, {channels})")
        work = DeviceBuffer((need,), np.uint8)
        out = new_output(n, channels)
        peak = 0.0 if self._normalize_peak is None else float(self._normalize_peak)
        check(lib().pgx_tralfam(out.ptr, snippet.dev.ptr, n, channels, self._seeded_generator().ptr, peak,
                                plan.buf.ptr, work.ptr), "pgx_tralfam")
        self._mogrified = out
        return out

    def _render(self, start: int, duration: int) -> Snippet:
        ext = self.extent()
        if ext.start is None or ext.end is None:
            return Snippet.from_zeros(start, duration, self.channel_count() or 1)
        mogrified = self._mogrify()
        frames, channels = mogrified.shape
        if start + duration <= ext.start or start >= ext.end:
            return Snippet.from_zeros(start, duration, channels)
        if ext.spans(start, duration):
            return Snippet.window_rows(start, mogrified, start - ext.start, duration)
        out = new_output(duration, channels)
        check(lib().pgx_window_copy(out.ptr, start, duration, channels, mogrified.ptr, ext.start, frames, 0, 0),
              "pgx_window_copy")
        return Snippet(start, out)

    def __repr__(self) -> str:
        parts = [f"source={self._source.__class__.__name__}"]
        if self._seed is not None:
            parts.append(f"seed={self._seed}")
        if self._normalize_peak is not None:
            parts.append(f"normalize_peak={self._normalize_peak}")
        return f"TralfamPE({', '.join(parts)})"
