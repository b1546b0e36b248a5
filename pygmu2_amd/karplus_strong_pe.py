"""
KarplusStrongPE: plucked string (karplus_strong_pe.py:61-220) and rho_for_decay_db (:22-58).

One period of float32 noise in a circular line, fed back through the two-point average times rho and a first-order
allpass for the fractional part of the period.  The line, its read position and the allpass state stay on the device
(pgx_karplus_strong, csrc/pgx_sources.hip) and the render runs the reference's float32 arithmetic in its order, so the
samples are bit for bit the reference's.  The excitation is drawn on the host with the reference's numpy expression at
the first render after a reset and uploaded once.  Like the reference, a render continues the string wherever it is:
a gap or a seek is not detected.
"""

from __future__ import annotations

import numpy as np

from . import device as _dev
from ._kernels import DeviceBuffer, check, lib, new_output
from .extent import Extent
from .snippet import Snippet
from .source_pe import SourcePE


def rho_for_decay_db(seconds: float, frequency: float, sample_rate: int, db: float = -60.0) -> float:
    """Feedback gain rho such that the string decays by |db| dB over `seconds` (karplus_strong_pe.py:22-58):
    rho = 10^(db / (20 * seconds * frequency)) / cos(pi / N), clamped to [1e-9, 1]."""
    periods = seconds * frequency
    if periods <= 0:
        raise ValueError("seconds * frequency must be positive")
    delay_len = max(2, int(np.floor(sample_rate / frequency)))
    avg_gain = np.cos(np.pi / delay_len)
    if avg_gain <= 0:
        return 1.0
    rho = float(10 ** (db / (20.0 * periods)) / avg_gain)
    return min(1.0, max(rho, 1e-9))


class KarplusStrongPE(SourcePE):
    _LOOK_AHEAD_SAFE = True            # contiguous renders are partition-invariant bit for bit (look_ahead.py)
    _STATE_FIELDS = ("_line", "_state", "_delay_len")

    def __init__(self, frequency: float, rho: float = 0.996, duration: int | None = None,
                 rho_damping: float | None = None, amplitude: float = 0.3, seed: int | None = None,
                 channels: int = 1):
        if frequency <= 0:
            raise ValueError(f"frequency must be positive, got {frequency}")
        if not (0 < rho <= 1.0):
            raise ValueError(f"rho must be in (0, 1], got {rho}")
        if amplitude <= 0:
            raise ValueError(f"amplitude must be positive, got {amplitude}")
        two_phase = duration is not None and rho_damping is not None
        if two_phase:
            if duration < 0:
                raise ValueError(f"duration must be >= 0, got {duration}")
            if not (0 < rho_damping <= 1.0):
                raise ValueError(f"rho_damping must be in (0, 1], got {rho_damping}")
        self._frequency = float(frequency)
        self._rho = float(rho)
        self._duration_param: int | None = duration if two_phase else None
        self._rho_damping: float | None = float(rho_damping) if two_phase else None
        self._amplitude = float(amplitude)
        self._seed = seed
        self._channels = channels
        self._line: DeviceBuffer | None = None      # (N,) float32; None until the first render after a reset
        self._state: DeviceBuffer | None = None     # one pgx_ks_state {r, ap_in, ap_out}
        self._delay_len = 0
        self._params: DeviceBuffer | None = None

    def _compute_extent(self) -> Extent:
        return Extent(0, None)

    def _reset_state(self) -> None:
        self._line = None

    def _on_start(self) -> None:
        self._reset_state()

    def _on_stop(self) -> None:
        self._reset_state()

    def _geometry(self) -> tuple[int, float]:
        """(N, allpass c) exactly as karplus_strong_pe.py:149-152 computes them."""
        delay_float = self.sample_rate / self._frequency
        delay_len = max(2, int(np.floor(delay_float)))
        frac_d = max(0.0, min(1.0, delay_float - delay_len))
        allpass_c = (1.0 - frac_d) / (1.0 + frac_d) if frac_d <= 1.0 else 0.0
        return delay_len, allpass_c

    def _excite(self) -> None:
        """The first render after a reset: one period of noise (:154-159), a zero allpass state, r = 0."""
        delay_len, allpass_c = self._geometry()
        rng = np.random.default_rng(self._seed)
        noise = rng.standard_normal(delay_len).astype(np.float32)
        noise *= self._amplitude / (np.max(np.abs(noise)) + 1e-9)
        self._line = DeviceBuffer.from_host(noise)
        self._state = DeviceBuffer((1,), _dev.KS_STATE, zero=True)
        self._delay_len = delay_len
        if self._params is None:
            rec = np.zeros(1, dtype=_dev.KS_PARAMS)
            rec[0] = (0, delay_len, int(self._duration_param is not None),
                      self._duration_param if self._duration_param is not None else 0,
                      np.float32(self._rho), np.float32(self._rho_damping or 0.0), np.float32(allpass_c), 0.0)
            self._params = _dev.upload_structs(rec)

    def _render(self, start: int, duration: int) -> Snippet:
        ch = self._channels
        ks_start, ks_end = max(0, start), max(0, start + duration)
        need = ks_end - ks_start
        out = new_output(duration, ch, zero=need < duration)
        if need <= 0:
            return Snippet(start, out)
        if self._line is None:
            self._excite()
        check(lib().pgx_karplus_strong(out.offset_ptr((ks_start - start) * ch), need * ch, 1, ks_start, need, ch,
                                       self._params.ptr, self._line.ptr, self._state.ptr, self._delay_len),
              "pgx_karplus_strong")
        return Snippet(start, out)

    def channel_count(self) -> int:
        return self._channels

    def is_pure(self) -> bool:
        return False

    def __repr__(self) -> str:
        if self._duration_param is not None and self._rho_damping is not None:
            return (f"KarplusStrongPE(frequency={self._frequency}, rho={self._rho}, "
                    f"duration={self._duration_param}, rho_damping={self._rho_damping})")
        return f"KarplusStrongPE(frequency={self._frequency}, rho={self._rho})"
