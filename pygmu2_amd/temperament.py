"""
Temperaments of the reference's temperament.py (:17-667): how a pitch number becomes a frequency and an interval a
frequency ratio.  Host math in float64 on array-likes, the reference's expressions in its order (the fixtures of
tests/golden/tuning_cases.json hold every function to an ulp), and its quirks as they are:

  * JustIntonation interpolates linearly in log2 between ratios[floor % N] and ratios[(floor + 1) % N]; the upper ratio
    is doubled when floor % N == N - 1 and the fraction is positive (temperament.py:372-402);
  * the scale degree  rel - floor(rel / N) * N  rounds to exactly N for a tiny negative rel: index N % N == 0 in the
    LOWER octave, so the frequency halves there;
  * JustIntonation.freq_to_pitch / ratio_to_interval give the nearest table entry (first minimum on a tie) of an input
    floored at 1e-10, never a fraction; their loop walks the rows of the input, so they take a list or an (n, 1) block
    and raise for a scalar or for rows of several channels (the device kernel has no such limit);
  * JustIntonation's pitch_to_freq / interval_to_ratio return shape (1,) for a scalar (np.atleast_1d inside),
    EqualTemperament's a 0-d result.

The module globals (temperament, reference frequency and pitch) are what the conversions of conversions.py and the
tuning descriptors of transforms.py use where nothing is passed.  `epoch()` counts their changes: TransformPE keeps the
device tables of a descriptor that follows the globals until it moves.

EqualTemperament and JustIntonation (PythagoreanTuning with it) also run on the device: `device_tuning()` is the record
pgx_tuning reads (include/pygmu_hip.h).  A CustomTemperament is the user's Python and stays on the host.
"""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import NamedTuple

import numpy as np

_FLOOR = 1e-10                     # the reference's guard in front of log2


class DeviceTuning(NamedTuple):
    """What one tuning step of pgx_tuning needs (pgx_tuning_record + its slice of the tables)."""
    just: bool                     # False: equal temperament
    reference_pitch: float         # equal: the reference pitch; just: the pitch of ratios[0]
    reference_freq: float          # equal: the reference frequency; just: the frequency of ratios[0] (base_freq)
    divisions: float               # equal: divisions per octave; just: len(ratios)
    table: np.ndarray | None       # just: log2(ratios), log2(ratios[0] * 2.0), then the ratios themselves


class Temperament(ABC):
    """pitch number <-> frequency, interval in scale degrees <-> frequency ratio."""

    @abstractmethod
    def pitch_to_freq(self, pitch, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        ...

    @abstractmethod
    def freq_to_pitch(self, freq, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        ...

    @abstractmethod
    def interval_to_ratio(self, interval):
        ...

    @abstractmethod
    def ratio_to_interval(self, ratio):
        ...

    @abstractmethod
    def name(self) -> str:
        ...

    def device_tuning(self, reference_pitch: float | None, reference_freq: float | None) -> DeviceTuning | None:
        """The record of this temperament for pgx_tuning (both None: the interval <-> ratio form), or None when the
        temperament is host code."""
        return None


class EqualTemperament(Temperament):
    """`divisions` equal steps per octave."""

    def __init__(self, divisions: int = 12):
        if divisions < 1:
            raise ValueError(f"Divisions must be positive, got {divisions}")
        self._divisions = divisions

    @property
    def divisions(self) -> int:
        return self._divisions

    def pitch_to_freq(self, pitch, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        pitch = np.asarray(pitch, dtype=np.float64)
        return reference_freq * (2.0 ** ((pitch - reference_pitch) / self._divisions))

    def freq_to_pitch(self, freq, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        freq = np.maximum(np.asarray(freq, dtype=np.float64), _FLOOR)
        return reference_pitch + self._divisions * np.log2(freq / reference_freq)

    def interval_to_ratio(self, interval):
        interval = np.asarray(interval, dtype=np.float64)
        return 2.0 ** (interval / self._divisions)

    def ratio_to_interval(self, ratio):
        ratio = np.maximum(np.asarray(ratio, dtype=np.float64), _FLOOR)
        return self._divisions * np.log2(ratio)

    def name(self) -> str:
        return f"{self._divisions}-tone Equal Temperament ({self._divisions}-ET)"

    def __repr__(self) -> str:
        return f"EqualTemperament(divisions={self._divisions})"

    def device_tuning(self, reference_pitch, reference_freq):
        if type(self) is not EqualTemperament:
            return None                                    # a subclass may compute anything
        if reference_pitch is None:                        # interval <-> ratio: x - 0.0, x / 1.0 and * 1.0 are exact
            return DeviceTuning(False, 0.0, 1.0, float(self._divisions), None)
        return DeviceTuning(False, float(reference_pitch), float(reference_freq), float(self._divisions), None)


_FIVE_LIMIT = [1.0, 16 / 15, 9 / 8, 6 / 5, 5 / 4, 4 / 3, 45 / 32, 3 / 2, 8 / 5, 5 / 3, 9 / 5, 15 / 8]
_PYTHAGOREAN = [1.0, 256 / 243, 9 / 8, 32 / 27, 81 / 64, 4 / 3, 1024 / 729, 3 / 2, 128 / 81, 27 / 16, 16 / 9, 243 / 128]


class JustIntonation(Temperament):
    """A table of frequency ratios for one octave (5-limit by default), `reference_pitch` the pitch of ratios[0];
    octaves transpose, fractional pitches interpolate in log-frequency."""

    def __init__(self, ratios=None, reference_pitch: float = 60.0):
        if ratios is None:
            self._ratios = np.array(_FIVE_LIMIT, dtype=np.float64)
        else:
            self._ratios = np.asarray(ratios, dtype=np.float64)
            if len(self._ratios) < 2:
                raise ValueError("Need at least 2 ratios (including unison)")
            if not np.isclose(self._ratios[0], 1.0):
                raise ValueError("First ratio must be 1.0 (unison)")
        self._reference_pitch = reference_pitch
        self._num_notes = len(self._ratios)

    @property
    def ratios(self) -> np.ndarray:
        return self._ratios.copy()

    @property
    def num_notes(self) -> int:
        return self._num_notes

    def _split(self, relative):
        """-> (octaves, scale degrees in [0, N]) of pitches relative to ratios[0]."""
        octaves = np.floor(relative / self._num_notes)
        return octaves, relative - octaves * self._num_notes

    def _interpolate_ratios(self, scale_degrees):
        scale_degrees = np.atleast_1d(scale_degrees)
        floor_idx = np.floor(scale_degrees).astype(int)
        frac = scale_degrees - floor_idx
        floor_idx = floor_idx % self._num_notes
        ceil_idx = (floor_idx + 1) % self._num_notes
        floor_ratios = self._ratios[floor_idx]
        ceil_ratios = self._ratios[ceil_idx]
        wrapped = (floor_idx == self._num_notes - 1) & (frac > 0)          # across the octave: the upper ratio doubles
        ceil_ratios = np.where(wrapped, ceil_ratios * 2.0, ceil_ratios)
        log_floor = np.log2(floor_ratios)
        log_ceil = np.log2(ceil_ratios)
        return 2.0 ** (log_floor + frac * (log_ceil - log_floor))

    def _base_freq(self, reference_pitch, reference_freq):
        """Frequency of ratios[0] when `reference_pitch` sounds at `reference_freq` (shape (1,))."""
        ref_octaves, ref_degree = self._split(reference_pitch - self._reference_pitch)
        ref_ratio = self._interpolate_ratios(ref_degree) * (2.0 ** ref_octaves)
        return reference_freq / ref_ratio

    def _nearest(self, ratio):
        """-> (octaves, index of the nearest table entry) of ratios >= 1e-10."""
        octaves = np.floor(np.log2(ratio))
        in_octave = ratio / (2.0 ** octaves)
        degrees = np.zeros_like(in_octave)
        for i, r in enumerate(np.atleast_1d(in_octave)):
            degrees[i] = np.argmin(np.abs(self._ratios - r))
        return octaves, degrees

    def pitch_to_freq(self, pitch, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        pitch = np.asarray(pitch, dtype=np.float64)
        octaves, degrees = self._split(pitch - self._reference_pitch)
        total_ratio = self._interpolate_ratios(degrees) * (2.0 ** octaves)
        return self._base_freq(reference_pitch, reference_freq) * total_ratio

    def freq_to_pitch(self, freq, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        freq = np.maximum(np.asarray(freq, dtype=np.float64), _FLOOR)
        octaves, degrees = self._nearest(freq / self._base_freq(reference_pitch, reference_freq))
        return self._reference_pitch + (octaves * self._num_notes + degrees)

    def interval_to_ratio(self, interval):
        interval = np.asarray(interval, dtype=np.float64)
        octaves, degrees = self._split(interval)
        return self._interpolate_ratios(degrees) * (2.0 ** octaves)

    def ratio_to_interval(self, ratio):
        ratio = np.maximum(np.asarray(ratio, dtype=np.float64), _FLOOR)
        octaves, degrees = self._nearest(ratio)
        return octaves * self._num_notes + degrees

    def name(self) -> str:
        return f"Just Intonation ({self._num_notes} notes)"

    def __repr__(self) -> str:
        return f"JustIntonation(num_notes={self._num_notes}, reference_pitch={self._reference_pitch})"

    def device_tuning(self, reference_pitch, reference_freq):
        if type(self) not in (JustIntonation, PythagoreanTuning):
            return None
        # numpy's own log2 bits; the extra entry is the doubled ratios[0] the reference takes across the octave
        table = np.concatenate([np.log2(self._ratios), [np.log2(self._ratios[0] * 2.0)], self._ratios])
        if reference_pitch is None:
            return DeviceTuning(True, 0.0, 1.0, float(self._num_notes), table)
        base = float(self._base_freq(reference_pitch, reference_freq)[0])
        return DeviceTuning(True, float(self._reference_pitch), base, float(self._num_notes), table)


class PythagoreanTuning(JustIntonation):
    """The 3-limit table: every interval from stacked 3:2 fifths."""

    def __init__(self, reference_pitch: float = 60.0):
        super().__init__(ratios=_PYTHAGOREAN, reference_pitch=reference_pitch)

    def name(self) -> str:
        return "Pythagorean Tuning"

    def __repr__(self) -> str:
        return f"PythagoreanTuning(reference_pitch={self._reference_pitch})"


class CustomTemperament(Temperament):
    """Four callables of the user's: p2f(pitch, reference_pitch, reference_freq), f2p(freq, reference_pitch,
    reference_freq), i2r(interval), r2i(ratio).  Results are returned as float64 arrays."""

    def __init__(self, pitch_to_freq_func, freq_to_pitch_func, interval_to_ratio_func, ratio_to_interval_func,
                 name: str = "Custom Temperament"):
        self._pitch_to_freq_func = pitch_to_freq_func
        self._freq_to_pitch_func = freq_to_pitch_func
        self._interval_to_ratio_func = interval_to_ratio_func
        self._ratio_to_interval_func = ratio_to_interval_func
        self._name = name

    def pitch_to_freq(self, pitch, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        return np.asarray(self._pitch_to_freq_func(pitch, reference_pitch, reference_freq), dtype=np.float64)

    def freq_to_pitch(self, freq, reference_pitch: float = 69.0, reference_freq: float = 440.0):
        return np.asarray(self._freq_to_pitch_func(freq, reference_pitch, reference_freq), dtype=np.float64)

    def interval_to_ratio(self, interval):
        return np.asarray(self._interval_to_ratio_func(interval), dtype=np.float64)

    def ratio_to_interval(self, ratio):
        return np.asarray(self._ratio_to_interval_func(ratio), dtype=np.float64)

    def name(self) -> str:
        return self._name

    def __repr__(self) -> str:
        return f"CustomTemperament(name='{self._name}')"


# ---------------------------------------------------------------------------------------------- the globals
_temperament: Temperament = EqualTemperament(12)
_reference_freq = 440.0
_reference_pitch = 69.0
_epoch = 0


def epoch() -> int:
    """Counts the changes of the globals below."""
    return _epoch


def set_temperament(temperament: Temperament) -> None:
    global _temperament, _epoch
    _temperament = temperament
    _epoch += 1


def get_temperament() -> Temperament:
    return _temperament


def set_reference_frequency(freq: float, pitch: float = 69.0) -> None:
    global _reference_freq, _reference_pitch, _epoch
    if freq <= 0:
        raise ValueError(f"Reference frequency must be positive, got {freq}")
    _reference_freq = float(freq)
    _reference_pitch = float(pitch)
    _epoch += 1


def get_reference_frequency() -> tuple[float, float]:
    """-> (reference frequency, reference pitch)."""
    return (_reference_freq, _reference_pitch)


def set_concert_pitch() -> None:
    set_reference_frequency(440.0, 69.0)


def set_verdi_tuning() -> None:
    set_reference_frequency(432.0, 69.0)


def set_baroque_pitch() -> None:
    set_reference_frequency(415.0, 69.0)
