"""
oracle/spec_builder.py -- TEST INFRASTRUCTURE ONLY.

The one interpreter of a golden-case SPEC (oracle/golden_cases.py) as a graph of PE instances.  It knows no PE class:
`K` is a flat namespace of the classes and enums named in TABLE plus three hooks,

    K.ExtendMode                         every "extend_mode" string goes through it
    K.transform_func(ops)                the callable a TransformPE gets for an op list
    K.hrtf(azimuth, elevation)           the SpatialHRTF method object, with the fixture's impulse responses at hand

so the same table builds over pygmu2_amd (tests/spec_build.namespace), over the reference's modules
(oracle/gen_golden.reference_namespace) and over recording stubs (tests/test_fixture_harness.py).

Children are built in `spec.items()` order before their parent: the fixtures list their PEs in construction order, and
some reference PEs draw from a global generator when they are constructed.
"""

from __future__ import annotations

from oracle.golden_cases import materialize_array


def is_spec(v):
    return isinstance(v, dict) and "pe" in v


def _mix(K, kw):
    return K.MixPE(*kw["inputs"])


def _piecewise(K, kw):
    kw["points"] = [(int(t), float(v)) for t, v in kw["points"]]
    return K.PiecewisePE(**kw)


def _spatial(K, kw):
    method = kw["method"]
    if method == "adapter":
        method = K.SpatialAdapter(kw["channels"])
    elif method == "linear":
        method = K.SpatialLinear(kw["azimuth"])
    elif method == "constant_power":
        method = K.SpatialConstantPower(kw["azimuth"])
    else:
        method = K.hrtf(kw["azimuth"], kw.get("elevation", 0.0))
    return K.SpatialPE(kw["source"], method=method)


def _transform(K, kw):
    return K.TransformPE(kw["source"], func=K.transform_func(kw["ops"]), name="ops")


def _row(enums=None, positional=(), make=None):
    """enums: keyword -> name of the enum in K that converts its string.  positional: the keywords passed as leading
    positional arguments, in order; a (keyword, default) pair is passed even where the SPEC leaves it out.  make(K, kw):
    a constructor call that is not `Class(*positional, **keywords)`."""
    return (enums or {}, positional, make)


PLAIN = _row()
TABLE = {
    "ConstantPE": PLAIN, "IdentityPE": PLAIN, "DiracPE": PLAIN, "ArrayPE": PLAIN, "CropPE": PLAIN, "SinePE": PLAIN,
    "GainPE": PLAIN, "BlitSawPE": PLAIN, "SuperSawPE": PLAIN, "CombPE": PLAIN, "AdsrGatedPE": PLAIN,
    "AdsrTriggeredPE": PLAIN, "PeriodicGate": PLAIN, "PeriodicTrigger": PLAIN, "KarplusStrongPE": PLAIN,
    "AnalogOscPE": PLAIN, "FunctionGenPE": PLAIN,
    "MixPE": _row(make=_mix),
    "PiecewisePE": _row(make=_piecewise),
    "SpatialPE": _row(make=_spatial),
    "TransformPE": _row(make=_transform),
    "BiquadPE": _row({"mode": "BiquadMode"}),
    "SVFilterPE": _row({"mode": "BiquadMode"}),
    "LadderPE": _row({"mode": "LadderMode"}),
    "EnvelopePE": _row({"mode": "DetectionMode"}),
    "WindowPE": _row({"mode": "WindowMode"}),
    "DynamicsPE": _row({"mode": "DynamicsMode"}),
    "NoisePE": _row({"mode": "NoiseMode"}),
    "DelayPE": _row({"interpolation": "InterpolationMode"}),
    "ConvolvePE": _row(positional=("src", "fir")),
    "ReverbPE": _row(positional=("source", "ir", ("mix", 0.5))),
    "LoopPE": _row(positional=("source",)),
    "CachePE": _row(positional=("source",)),
    "TriggerRestartPE": _row(positional=("trigger", "src")),
    "CompressorPE": _row({"detection": "DetectionMode"}, ("source",)),
    "LimiterPE": _row({"detection": "DetectionMode"}, ("source",)),
    "ExpanderPE": _row({"detection": "DetectionMode"}, ("source",)),
    "WavetablePE": _row({"interpolation": "InterpolationMode", "out_of_bounds": "OutOfBoundsMode"},
                        ("wavetable", "indexer")),
    "TimeWarpPE": _row({"interpolation": "InterpolationMode"}, ("source",)),
    "SampleHoldPE": _row(positional=("source", "trigger")),
    "TrackHoldPE": _row(positional=("source", "gate")),
    "SlewLimiterPE": _row({"mode": "SlewMode"}, ("source",)),
}


def build(spec, K, shared=None, on_make=None):
    """SPEC -> PE instance over the namespace K.  A node with `"share": <name>` is one instance wherever the name
    appears (`shared` carries them).  on_make(kind, pe) is called for every node constructed, in construction order."""
    shared = {} if shared is None else shared
    name = spec.get("share")
    if name is not None and name in shared:
        return shared[name]
    kind = spec["pe"]
    enums, positional, make = TABLE[kind]
    kw = {}
    for k, v in spec.items():
        if k in ("pe", "share"):
            continue
        if is_spec(v):
            kw[k] = build(v, K, shared, on_make)
        elif isinstance(v, dict):
            kw[k] = materialize_array(v)
        elif k == "inputs":
            kw[k] = [build(s, K, shared, on_make) for s in v]
        else:
            kw[k] = v
    for k, enum in dict(enums, extend_mode="ExtendMode").items():
        if k in kw:
            kw[k] = getattr(K, enum)(kw[k])
    if make is not None:
        pe = make(K, kw)
    else:
        args = [kw.pop(*p) if isinstance(p, tuple) else kw.pop(p) for p in positional]
        pe = getattr(K, kind)(*args, **kw)
    if on_make is not None:
        on_make(kind, pe)
    if name is not None:
        shared[name] = pe
    return pe


def kinds_of(spec, out=None):
    """The set of kinds a SPEC (or a list of SPECs) names, at any depth."""
    out = set() if out is None else out
    if isinstance(spec, dict):
        if "pe" in spec:
            out.add(spec["pe"])
        for v in spec.values():
            kinds_of(v, out)
    elif isinstance(spec, list):
        for v in spec:
            kinds_of(v, out)
    return out
