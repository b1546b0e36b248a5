"""
Named element-wise transforms for TransformPE.

The reference's TransformPE (transform_pe.py:19-66) takes an arbitrary Python callable
over numpy arrays.  A callable cannot cross the C ABI, so the common shapes are offered as
small descriptor objects that TransformPE lowers to one device kernel (pgx_transform).
Every descriptor is also a plain numpy callable with the same float64 arithmetic, so the
same object can be handed to the reference's TransformPE.

    Affine(scale, offset)   offset + scale * x          Abs()        |x|
    Clip(lo, hi)            np.clip(x, lo, hi)          Tanh()       np.tanh(x)
    Sqrt()                  x ** 0.5                    OneMinus()   1.0 - x
    Square()                x ** 2                      Chain(a, b, ...)  b(a(x)) ...

The tuning steps are descriptors too -- their __call__ is the matching function of conversions.py -- and a chain that
holds one runs in pgx_tuning, still one kernel and one rounding:

    PitchToFreq(temperament=None, reference_pitch=None, reference_freq=None)      SemitonesToRatio(temperament=None)
    FreqToPitch(temperament=None, reference_pitch=None, reference_freq=None)      RatioToSemitones(temperament=None)

None follows the globals of temperament.py, read whenever a block is rendered.  lower() turns the four conversions
functions themselves, and a functools.partial of one with keyword arguments only, into these.  A step over a
CustomTemperament is the user's Python: not lowered.
"""

from __future__ import annotations

import functools

import numpy as np

from . import conversions as _conv
from . import temperament as _tm

AFFINE, CLIP, SQRT, SQUARE, ABS, TANH, ONE_MINUS = range(7)
# pgx_tuning's codes: an op of these is (code, temperament.DeviceTuning, 0.0)
ET_PITCH_TO_FREQ, ET_FREQ_TO_PITCH, JI_PITCH_TO_FREQ, JI_FREQ_TO_PITCH = range(7, 11)
TUNING_CODES = (ET_PITCH_TO_FREQ, ET_FREQ_TO_PITCH, JI_PITCH_TO_FREQ, JI_FREQ_TO_PITCH)


class DeviceTransform:
    """Base class: `ops()` lists (code, p0, p1) triples in application order."""

    def ops(self) -> list[tuple[int, float, float]]:
        raise NotImplementedError

    def __call__(self, v):
        raise NotImplementedError

    def lowerable(self) -> bool:
        """False: this descriptor can only run as a host callable (a tuning step bound to host code)."""
        return True

    def follows_globals(self) -> bool:
        """True: ops() depends on temperament.py's globals, so it is asked again when they have changed."""
        return False

    @property
    def __name__(self) -> str:        # TransformPE's default display name
        return type(self).__name__.lower()


class Affine(DeviceTransform):
    def __init__(self, scale: float = 1.0, offset: float = 0.0):
        self.scale, self.offset = float(scale), float(offset)

    def ops(self):
        return [(AFFINE, self.scale, self.offset)]

    def __call__(self, v):
        return self.offset + self.scale * v


class Clip(DeviceTransform):
    def __init__(self, lo: float, hi: float):
        if lo > hi:
            raise ValueError(f"Clip: lo ({lo}) > hi ({hi})")
        self.lo, self.hi = float(lo), float(hi)

    def ops(self):
        return [(CLIP, self.lo, self.hi)]

    def __call__(self, v):
        return np.clip(v, self.lo, self.hi)


class _Unary(DeviceTransform):
    code = -1

    def ops(self):
        return [(self.code, 0.0, 0.0)]


class Sqrt(_Unary):
    code = SQRT

    def __call__(self, v):
        return v ** 0.5


class Square(_Unary):
    code = SQUARE

    def __call__(self, v):
        return v ** 2


class Abs(_Unary):
    code = ABS

    def __call__(self, v):
        return np.abs(v)


class Tanh(_Unary):
    code = TANH

    def __call__(self, v):
        return np.tanh(v)


class OneMinus(_Unary):
    code = ONE_MINUS

    def __call__(self, v):
        return 1.0 - v


class Chain(DeviceTransform):
    def __init__(self, *steps: DeviceTransform):
        for s in steps:
            if not isinstance(s, DeviceTransform):
                raise TypeError(f"Chain takes DeviceTransform steps, got {type(s).__name__}")
        self.steps = steps

    def ops(self):
        return [op for s in self.steps for op in s.ops()]

    def __call__(self, v):
        for s in self.steps:
            v = s(v)
        return v

    def lowerable(self):
        return all(s.lowerable() for s in self.steps)

    def follows_globals(self):
        return any(s.follows_globals() for s in self.steps)


class _TuningStep(DeviceTransform):
    """One of the four conversions.  ops() resolves whatever is None from the globals NOW; when that lands on host code
    (a CustomTemperament set globally) it raises LookupError and TransformPE runs __call__ on the host."""
    _with_reference = True             # pitch <-> frequency; False: interval <-> ratio
    _inverse = False                   # frequency -> pitch / ratio -> interval
    _function = None

    def __init__(self, temperament=None, reference_pitch=None, reference_freq=None):
        if temperament is not None:
            _conv._resolve(temperament)                    # the conversions' own refusal of anything else
        self.temperament = temperament
        self.reference_pitch = None if reference_pitch is None else float(reference_pitch)
        self.reference_freq = None if reference_freq is None else float(reference_freq)

    def _keywords(self) -> dict:
        if not self._with_reference:
            return {"temperament": self.temperament}
        return {"temperament": self.temperament, "reference_pitch": self.reference_pitch,
                "reference_freq": self.reference_freq}

    def __call__(self, v):
        return type(self)._function(v, **self._keywords())

    def follows_globals(self):
        return any(value is None for value in self._keywords().values())

    def lowerable(self):
        return self.temperament is None or self.temperament.device_tuning(None, None) is not None

    def ops(self):
        temp = _conv._resolve(self.temperament)
        if self._with_reference:
            tuning = temp.device_tuning(*_conv._reference(self.reference_pitch, self.reference_freq))
        else:
            tuning = temp.device_tuning(None, None)
        if tuning is None:
            raise LookupError(f"{temp!r} is host code")
        code = (JI_PITCH_TO_FREQ if tuning.just else ET_PITCH_TO_FREQ) + int(self._inverse)
        return [(code, tuning, 0.0)]

    def __repr__(self) -> str:
        inner = ", ".join(f"{k}={v!r}" for k, v in self._keywords().items())
        return f"{type(self).__name__}({inner})"


class PitchToFreq(_TuningStep):
    _function = staticmethod(_conv.pitch_to_freq)


class FreqToPitch(_TuningStep):
    _inverse = True
    _function = staticmethod(_conv.freq_to_pitch)


class SemitonesToRatio(_TuningStep):
    _with_reference = False
    _function = staticmethod(_conv.semitones_to_ratio)

    def __init__(self, temperament=None):
        super().__init__(temperament)


class RatioToSemitones(_TuningStep):
    _with_reference = False
    _inverse = True
    _function = staticmethod(_conv.ratio_to_semitones)

    def __init__(self, temperament=None):
        super().__init__(temperament)


# numpy callables that mean the same thing as a descriptor
_NUMPY_EQUIVALENTS = {np.abs: Abs, np.absolute: Abs, np.fabs: Abs, np.tanh: Tanh, np.sqrt: Sqrt,
                      np.square: Square}


# the conversions functions that mean the same thing as a tuning descriptor
_CONVERSIONS = {_conv.pitch_to_freq: PitchToFreq, _conv.freq_to_pitch: FreqToPitch,
                _conv.semitones_to_ratio: SemitonesToRatio, _conv.ratio_to_semitones: RatioToSemitones}


def lower(func):
    """DeviceTransform for `func`, or None when it is an opaque Python callable."""
    if isinstance(func, DeviceTransform):
        return func if func.lowerable() else None
    keywords = {}
    if isinstance(func, functools.partial):
        if func.args:                 # a bound positional argument would be the stream itself
            return None
        func, keywords = func.func, func.keywords
    try:
        cls = _NUMPY_EQUIVALENTS.get(func) if not keywords else None
        tuning = _CONVERSIONS.get(func)
    except TypeError:                 # unhashable callable
        return None
    if tuning is not None:
        try:
            step = tuning(**keywords)
        except (TypeError, NotImplementedError):          # keywords the conversion does not take: its own error, on the host
            return None
        return step if step.lowerable() else None
    return cls() if cls is not None else None


def from_spec(ops) -> Chain:
    """[(name, *params), ...] (the golden-case notation of oracle/golden_cases.py) -> Chain."""
    table = {"affine": Affine, "clip": Clip, "sqrt": Sqrt, "square": Square, "abs": Abs, "tanh": Tanh,
             "one_minus": OneMinus}
    tuning = {"pitch_to_freq": PitchToFreq, "freq_to_pitch": FreqToPitch, "semitones_to_ratio": SemitonesToRatio,
              "ratio_to_semitones": RatioToSemitones}

    def step(op):
        if op[0] in tuning:           # [name, temperament spec or None, reference_pitch, reference_freq]
            return tuning[op[0]](temperament_from_spec(op[1] if len(op) > 1 else None), *op[2:])
        return table[op[0]](*op[1:])
    return Chain(*(step(op) for op in ops))


def temperament_from_spec(spec):
    """{"kind": "equal", "divisions": 19} | {"kind": "just", "ratios": [...] or None, "reference_pitch": 60.0} |
    {"kind": "pythagorean", "reference_pitch": 60.0} | None (the global one) -> Temperament or None."""
    if spec is None:
        return None
    kind = spec["kind"]
    if kind == "equal":
        return _tm.EqualTemperament(int(spec.get("divisions", 12)))
    if kind == "just":
        return _tm.JustIntonation(spec.get("ratios"), spec.get("reference_pitch", 60.0))
    if kind == "pythagorean":
        return _tm.PythagoreanTuning(spec.get("reference_pitch", 60.0))
    raise ValueError(f"unknown temperament kind {kind!r}")
