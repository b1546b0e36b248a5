"""
Unit conversions of the reference's conversions.py (:21-109, :168-281): pitch number <-> frequency, semitones <->
frequency ratio, samples <-> seconds.  Host math in float64 on array-likes, the reference's expressions in its order,
for its default tuning only: 12-tone equal temperament, A4 = pitch 69 = 440 Hz (temperament.py:137-167).  The
temperament classes are not part of this package: any `temperament=` other than None raises NotImplementedError.
ratio_to_db / db_to_ratio live in dynamics_pe.py.
"""

from __future__ import annotations

import numpy as np

_DIVISIONS = 12
_REFERENCE_PITCH = 69.0
_REFERENCE_FREQ = 440.0
_FLOOR = 1e-10                     # the reference's guard in front of log2


def _default_tuning_only(temperament) -> None:
    if temperament is not None:
        raise NotImplementedError(
            "pygmu2_amd has no temperament module: only the default tuning (12-tone equal temperament, "
            "A4 = 69 = 440 Hz) is available; pass temperament=None")


def pitch_to_freq(pitch, temperament=None):
    """Frequency in Hz of a (possibly fractional) MIDI pitch number."""
    _default_tuning_only(temperament)
    pitch = np.asarray(pitch, dtype=np.float64)
    return _REFERENCE_FREQ * (2.0 ** ((pitch - _REFERENCE_PITCH) / _DIVISIONS))


def freq_to_pitch(freq, temperament=None):
    """MIDI pitch number of a frequency in Hz."""
    _default_tuning_only(temperament)
    freq = np.maximum(np.asarray(freq, dtype=np.float64), _FLOOR)
    return _REFERENCE_PITCH + _DIVISIONS * np.log2(freq / _REFERENCE_FREQ)


def semitones_to_ratio(semitones, temperament=None):
    """Frequency ratio of an interval in semitones (12 -> 2.0)."""
    _default_tuning_only(temperament)
    semitones = np.asarray(semitones, dtype=np.float64)
    return 2.0 ** (semitones / _DIVISIONS)


def ratio_to_semitones(ratio, temperament=None):
    """Interval in semitones of a frequency ratio (2.0 -> 12)."""
    _default_tuning_only(temperament)
    ratio = np.maximum(np.asarray(ratio, dtype=np.float64), _FLOOR)
    return _DIVISIONS * np.log2(ratio)


def samples_to_seconds(samples, sample_rate):
    return np.asarray(samples, dtype=np.float64) / sample_rate


def seconds_to_samples(seconds, sample_rate):
    """Float sample count: the caller rounds."""
    return np.asarray(seconds, dtype=np.float64) * sample_rate
