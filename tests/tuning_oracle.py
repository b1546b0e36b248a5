"""The tuning family's fixture format (tests/golden/tuning_cases.json + tuning.npz), shared by its generator
(tools/gen_golden_tuning.py, over the reference's classes) and its tests (over pygmu2_amd's): temperaments from their
specs, the graph builder, the block loop with this family's "tuning" verb, and the clearance rule of the just
freq -> pitch streams.  The numpy restatement the generator holds the reference's records to is pygmu2_amd.temperament
itself (host code, no device)."""

from __future__ import annotations

import functools
import types

import numpy as np

import fixture_harness as H

EDGE_CLEARANCE = 1e-9          # just freq -> pitch: log2(ratio) from an integer, and the two smallest |ratios - r| apart
FUNCTIONS = ("pitch_to_freq", "freq_to_pitch", "semitones_to_ratio", "ratio_to_semitones")


def package_namespace():
    """pygmu2_amd as the namespace build_graph works over."""
    import pygmu2_amd as pg
    from pygmu2_amd import transforms
    M = types.SimpleNamespace(**{k: getattr(pg, k) for k in dir(pg) if not k.startswith("_")})
    M.transform = lambda ops: transforms.from_spec(ops)
    return M


def temperament(M, spec):
    """{"kind": "equal" | "just" | "pythagorean", ...} (transforms.temperament_from_spec's notation) over M's classes."""
    if spec is None:
        return None
    if spec["kind"] == "equal":
        return M.EqualTemperament(int(spec.get("divisions", 12)))
    if spec["kind"] == "just":
        return M.JustIntonation(spec.get("ratios"), spec.get("reference_pitch", 60.0))
    assert spec["kind"] == "pythagorean", spec
    return M.PythagoreanTuning(spec.get("reference_pitch", 60.0))


def numpy_chain(M, ops):
    """The callable a user of the reference passes to TransformPE for an op list of transforms.from_spec's notation."""
    def f(v):
        for op in ops:
            if op[0] == "affine":
                v = op[2] + op[1] * v
            elif op[0] == "clip":
                v = np.clip(v, op[1], op[2])
            elif op[0] in ("pitch_to_freq", "freq_to_pitch"):
                v = getattr(M, op[0])(v, temperament(M, op[1]), *op[2:])
            else:
                assert op[0] in ("semitones_to_ratio", "ratio_to_semitones"), op
                v = getattr(M, op[0])(v, temperament(M, op[1]))
        return v
    return f


def _keywords(M, kw):
    kw = dict(kw)
    if "temperament" in kw:
        kw["temperament"] = temperament(M, kw["temperament"])
    return kw


def build_graph(M, spec):
    """A JSON graph spec over the namespace M.  {"type": <class of M>, "args": [...], "kwargs": {...}} and
      {"type": "Transform", "source": g, "ops": [...]}                  TransformPE(g, func=M.transform(ops))
      {"type": "Transform", "source": g, "func": name}                  TransformPE(g, func=M.<name>): the function itself
      {"type": "Transform", "source": g, "func": name, "partial": kw}   ... functools.partial(M.<name>, **kw)
      {"type": "Freq", "pitch": p, "keywords": kw}                      the value M.pitch_to_freq(p, **kw), not a PE
      {"type": "Array", "seed": s, "n": n, "ch": c, "lo": a, "hi": b}   ArrayPE of float32 uniform noise
    Enum values are given by name: {"enum": "TransitionType", "name": "STEP"}."""
    if isinstance(spec, list):
        return [build_graph(M, s) for s in spec]
    if not isinstance(spec, dict):
        return spec
    if "enum" in spec:
        return getattr(getattr(M, spec["enum"]), spec["name"])
    t = spec["type"]
    if t == "Transform":
        src = build_graph(M, spec["source"])
        if "ops" in spec:
            return M.TransformPE(src, func=M.transform(spec["ops"]))
        func = getattr(M, spec["func"])
        if "partial" in spec:
            func = functools.partial(func, **_keywords(M, spec["partial"]))
        return M.TransformPE(src, func=func)
    if t == "Freq":
        return M.pitch_to_freq(spec["pitch"], **_keywords(M, spec.get("keywords", {})))
    if t == "Array":
        return M.ArrayPE(array_data(spec))
    args = [build_graph(M, a) for a in spec.get("args", [])]
    kwargs = {k: build_graph(M, v) for k, v in spec.get("kwargs", {}).items()}
    if t == "PiecewisePE":
        args[0] = [(int(p[0]), float(p[1])) for p in args[0]]
    return getattr(M, t)(*args, **kwargs)


def array_data(spec):
    rng = np.random.default_rng(int(spec["seed"]))
    return rng.uniform(spec["lo"], spec["hi"], (int(spec["n"]), int(spec["ch"]))).astype(np.float32)


def set_tuning(M, tuning):
    """The "tuning" verb: {"temperament": spec} and / or {"reference": [freq, pitch]} become the globals."""
    if tuning.get("temperament") is not None:
        M.set_temperament(temperament(M, tuning["temperament"]))
    if tuning.get("reference") is not None:
        M.set_reference_frequency(*tuning["reference"])


def default_tuning(M):
    M.set_temperament(M.EqualTemperament(12))
    M.set_concert_pitch()


def render_case(M, case, renderer):
    """Every block of a case in a started renderer -> list of float32 arrays.  case["ops"] = {block index:
    {"tuning": ...}}: the globals change before that block, as a user calling set_temperament between two renders;
    they are the defaults before the first block and again afterwards."""
    default_tuning(M)
    pe = build_graph(M, case["graph"])
    ops, at = case.get("ops", {}), [0]

    def render(start, n):
        op = ops.get(str(at[0]))
        at[0] += 1
        if op is not None:
            set_tuning(M, op["tuning"])
        return np.array(pe.render(start, n).data, dtype=np.float32)
    try:
        return H.render_blocks(pe, case["sr"], case["blocks"], renderer=renderer, render=render)
    finally:
        default_tuning(M)


def call_function(M, rec, values):
    """One "functions" record through M's conversions."""
    temp = temperament(M, rec["temperament"])
    if rec["fn"] in ("pitch_to_freq", "freq_to_pitch"):
        freq, pitch = rec["reference"]
        return getattr(M, rec["fn"])(values, temperament=temp, reference_pitch=pitch, reference_freq=freq)
    return getattr(M, rec["fn"])(values, temperament=temp)


def shape_of(fn, value):
    """[type name, shape, dtype] of fn(value), or ["raises", exception type] -- the reference's nearest-entry loop
    indexes a 0-d array for a scalar."""
    try:
        out = fn(value)
    except Exception as e:                                       # noqa: BLE001  (whatever the reference raises is the fact)
        return ["raises", type(e).__name__]
    return [type(out).__name__, list(np.shape(out)), str(np.asarray(out).dtype)]


def just_clearance(ratios, ratio):
    """-> (distance of log2(ratio) from an integer, gap between the two smallest |ratios - r|), the minima over the
    samples: what a just freq -> pitch result is decided by."""
    ratio = np.maximum(np.asarray(ratio, dtype=np.float64).reshape(-1), 1e-10)
    lg = np.log2(ratio)
    octave = np.floor(lg)
    r = ratio / 2.0 ** octave
    d = np.sort(np.abs(np.asarray(ratios, dtype=np.float64)[None, :] - r[:, None]), axis=1)
    return float(np.min(np.abs(lg - np.rint(lg)))), float(np.min(d[:, 1] - d[:, 0]))
