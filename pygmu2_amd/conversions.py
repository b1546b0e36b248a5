"""
Unit conversions of the reference's conversions.py (:21-109, :168-281): pitch number <-> frequency, semitones <->
frequency ratio, samples <-> seconds.  Host math in float64 on array-likes, the reference's expressions in its order.

The four tuning conversions take a `temperament=` (an instance of temperament.Temperament: EqualTemperament,
JustIntonation, PythagoreanTuning, CustomTemperament or a subclass of the user's) and pitch_to_freq / freq_to_pitch a
`reference_pitch=` / `reference_freq=`; whatever is None is read from the globals of temperament.py when the function is
called (set_temperament, set_reference_frequency: 12-tone equal temperament, A4 = pitch 69 = 440 Hz until changed).
Anything else passed as `temperament=` raises NotImplementedError.  TransformPE runs these four on the device
(transforms.PitchToFreq ...).  ratio_to_db / db_to_ratio live in dynamics_pe.py.
"""

from __future__ import annotations

import numpy as np

from . import temperament as _tm


def _resolve(temperament) -> _tm.Temperament:
    if temperament is None:
        return _tm.get_temperament()
    if not isinstance(temperament, _tm.Temperament):
        raise NotImplementedError(
            f"temperament= takes an instance of pygmu2_amd.temperament.Temperament (EqualTemperament, JustIntonation, "
            f"PythagoreanTuning, CustomTemperament) or None for the global one, not {type(temperament).__name__}")
    return temperament


def _reference(reference_pitch, reference_freq) -> tuple[float, float]:
    if reference_freq is None or reference_pitch is None:
        global_freq, global_pitch = _tm.get_reference_frequency()
        reference_freq = global_freq if reference_freq is None else reference_freq
        reference_pitch = global_pitch if reference_pitch is None else reference_pitch
    return reference_pitch, reference_freq


def pitch_to_freq(pitch, temperament=None, reference_pitch=None, reference_freq=None):
    """Frequency in Hz of a (possibly fractional) pitch number."""
    temp = _resolve(temperament)
    reference_pitch, reference_freq = _reference(reference_pitch, reference_freq)
    return temp.pitch_to_freq(pitch, reference_pitch, reference_freq)


def freq_to_pitch(freq, temperament=None, reference_pitch=None, reference_freq=None):
    """Pitch number of a frequency in Hz."""
    temp = _resolve(temperament)
    reference_pitch, reference_freq = _reference(reference_pitch, reference_freq)
    return temp.freq_to_pitch(freq, reference_pitch, reference_freq)


def semitones_to_ratio(semitones, temperament=None):
    """Frequency ratio of an interval in scale degrees of the temperament (12-ET: 12 -> 2.0)."""
    return _resolve(temperament).interval_to_ratio(semitones)


def ratio_to_semitones(ratio, temperament=None):
    """Interval in scale degrees of the temperament of a frequency ratio (12-ET: 2.0 -> 12)."""
    return _resolve(temperament).ratio_to_interval(ratio)


def samples_to_seconds(samples, sample_rate):
    return np.asarray(samples, dtype=np.float64) / sample_rate


def seconds_to_samples(seconds, sample_rate):
    """Float sample count: the caller rounds."""
    return np.asarray(seconds, dtype=np.float64) * sample_rate
