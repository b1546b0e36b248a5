#!/usr/bin/env python3
"""
oracle/gen_golden.py -- TEST INFRASTRUCTURE ONLY; runs ONLY in the build container,
where the read-only reference tree exists at /root/reference.

Imports the reference's PE modules (bare-package loader: the package __init__ pulls
soundfile/sounddevice which are absent; numba is replaced by a pass-through decorator
so the *_numba kernel bodies run as plain Python, i.e. the block-size-invariant numba
semantics), builds every case of oracle/golden_cases.py with
the reference's own classes, renders the listed blocks through a started
NullRenderer graph and writes

    tests/golden/cases.json      (case list: graph SPECs, blocks, sample rate)
    tests/golden/golden.npz      (float32 outputs, key "<case>/<block index>")

Only data (inputs are regenerated from the SPEC, outputs are stored) goes into the
repository; no reference source text is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python3 oracle/gen_golden.py
"""

from __future__ import annotations

import importlib
import json
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
REF = "/root/reference/src/pygmu2"

from oracle import spec_builder  # noqa: E402
from oracle.golden_cases import S, cases  # noqa: E402


def load_reference():
    logging.disable(logging.CRITICAL)

    def _passthrough(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    nb = types.ModuleType("numba")
    nb.jit = _passthrough
    nb.njit = _passthrough
    sys.modules["numba"] = nb
    # spatial_pe imports soundfile (absent) at module level; only SpatialHRTF._load_ir calls it, and the
    # HRTF cases pre-fill the instance's IR cache from the fixture WAVs, so an empty module is enough
    sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
    pkg = types.ModuleType("pygmu2")
    pkg.__path__ = [REF]
    sys.modules["pygmu2"] = pkg
    mods = {}
    for name in ("config", "extent", "snippet", "null_renderer", "constant_pe", "identity_pe",
                 "dirac_pe", "array_pe", "crop_pe", "sine_pe", "gain_pe", "mix_pe", "biquad_pe",
                 "blit_saw_pe", "super_saw_pe", "ladder_pe", "comb_pe", "adsr_pe",
                 "periodic_gate", "periodic_trigger", "convolve_pe", "svfilter_pe", "envelope_pe",
                 "transform_pe", "wavetable_pe", "delay_pe", "piecewise_pe", "trigger_restart_pe", "cache_pe",
                 "reverb_pe", "assets", "spatial_pe", "loop_pe", "window_pe", "conversions", "dynamics_pe",
                 "compressor_pe", "karplus_strong_pe", "analog_osc_pe"):
        mods[name] = importlib.import_module(f"pygmu2.{name}")
    mods["K"] = reference_namespace(mods)
    return mods


# modules beside load_reference()'s that the newer families' generators read classes from
EXTRA_MODULES = ("timewarp_pe", "sample_hold_pe", "track_hold_pe", "slew_limiter_pe", "function_gen_pe", "noise_pe",
                 "tralfam_pe", "slice_pe", "set_extent_pe", "sequence_pe")


def reference_namespace(M):
    """The reference's classes and enums as the flat namespace oracle/spec_builder.py builds over (every capitalised
    name of load_reference()'s modules and of EXTRA_MODULES), with the builder's hooks."""
    K = types.SimpleNamespace()
    for mod in list(M.values()) + [importlib.import_module(f"pygmu2.{name}") for name in EXTRA_MODULES]:
        for name, value in vars(mod).items():
            if name[:1].isupper() and getattr(value, "__module__", None) == mod.__name__:
                setattr(K, name, value)
    K.transform_func = numpy_func
    K.hrtf = lambda azimuth, elevation: hrtf_method(K.SpatialHRTF, azimuth, elevation)
    return K


def hrtf_method(SpatialHRTF, azimuth, elevation):
    """A SpatialHRTF whose IR cache holds the fixture WAV it would load (the reference reads it through soundfile)."""
    import wave
    meth = SpatialHRTF(azimuth, elevation)
    name = SpatialHRTF.hrtf_filename_for(meth.azimuth, meth.elevation)
    with wave.open(os.path.join(ROOT, "tests", "golden", "kemar", name), "rb") as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, w.getnchannels())
        # libsndfile's PCM16 -> float32 (x / 32768), what sf.read(dtype="float32") returns
        meth._ir_cache[name] = ((pcm.astype(np.float32) * np.float32(1.0 / 32768.0)), w.getframerate())
    return meth


def build(spec, M, shared=None, on_make=None):
    """SPEC -> reference PE instance: oracle/spec_builder.py's table over the namespace of load_reference()."""
    return spec_builder.build(spec, M["K"], shared, on_make)


def numpy_func(ops):
    """The plain numpy callable a reference user would pass to TransformPE for this op list."""
    def f(v):
        for op in ops:
            name = op[0]
            if name == "affine":
                v = op[2] + op[1] * v
            elif name == "clip":
                v = np.clip(v, op[1], op[2])
            elif name == "sqrt":
                v = v ** 0.5
            elif name == "square":
                v = v ** 2
            elif name == "abs":
                v = np.abs(v)
            elif name == "tanh":
                v = np.tanh(v)
            elif name == "one_minus":
                v = 1.0 - v
            else:
                raise KeyError(name)
        return v
    return f


def has_kind(spec, kind):
    return kind in spec_builder.kinds_of(spec)


def render_case(case, M):
    """Every block of a case (the format of oracle/golden_cases.py) through the reference's classes, in a started
    NullRenderer -> list of float32 arrays."""
    M["config"].set_sample_rate(case["sr"])
    pe = build(case["graph"], M)
    r = M["null_renderer"].NullRenderer(sample_rate=case["sr"])
    r.set_source(pe)
    # A reference ConvolvePE cannot be start()ed (its _reset_state drops the tail
    # that _ensure_filter_prepared never re-creates); the
    # reference's own tests render it un-started, so do the same.
    if not (has_kind(case["graph"], "ConvolvePE") or has_kind(case["graph"], "ReverbPE")):
        r.start()
    outs = []
    for s, n in case["blocks"]:
        data = pe.render(int(s), int(n)).data
        assert data.dtype == np.float32 and data.shape[0] == n, (case["name"], data.dtype, data.shape)
        outs.append(np.ascontiguousarray(data))
    return outs


# ---------------------------------------------------------------------------------------------- shared by tools/gen_golden_*.py
def affine(src, scale, offset):
    return S("TransformPE", source=src, ops=[["affine", scale, offset]])


def sums_exact(values):
    """True when every sum of any of these float64 values, in any order, is exact: all are multiples of 2^-q and the
    sum of their magnitudes times 2^q stays below 2^52."""
    values = np.asarray(values, dtype=np.float64)
    if not np.all(np.isfinite(values)):
        return False
    for q in range(0, 41):
        scaled = values * 2.0 ** q
        if np.all(scaled == np.round(scaled)):
            return float(np.sum(np.abs(scaled))) < 2.0 ** 52
    return False


def render_reference(case, M, kinds, reset=None, render=None):
    """A case with lifecycle "ops" through the reference's classes, by tests/fixture_harness.render_blocks
    -> (blocks, root PE, its PEs of `kinds` in construction order).  reset(made): what a "reset" op does (reset_state()
    of every one of them by default); render(pe, made, start, n): another way to pull one block."""
    import fixture_harness as H
    made = []
    pe = build(case["graph"], M, on_make=lambda kind, node: made.append(node) if kind in kinds else None)
    outs = H.render_blocks(pe, case["sr"], case["blocks"], case.get("ops"), lambda: (reset or H.reset_all)(made),
                           renderer=M["null_renderer"].NullRenderer(sample_rate=case["sr"]),
                           render=render and (lambda s, n: render(pe, made, s, n)))
    return outs, pe, made


def describe(pe):
    """What the reference says about a PE, for the host-side tests."""
    ext = pe.extent()
    return {"repr": repr(pe), "extent": [ext.start, ext.end], "pure": bool(pe.is_pure()),
            "channels": pe.channel_count(), "inputs": [type(i).__name__ for i in pe.inputs()]}


def write_fixture(family, doc, arrays):
    """tests/golden/<family>_cases.json and <family>.npz."""
    import fixture_harness as H
    cases_path, npz_path = H.paths(family)
    with open(cases_path, "w") as fh:
        json.dump(doc, fh, indent=1)
    np.savez_compressed(npz_path, **arrays)
    print(npz_path, os.path.getsize(npz_path), "bytes,", sum(a.size for a in arrays.values()), "samples;", cases_path,
          os.path.getsize(cases_path), "bytes")


def main():
    M = load_reference()
    out = {}
    case_list = cases()
    for case in case_list:
        outs = render_case(case, M)
        for i in case["keep"]:
            out[f"{case['name']}/{i}"] = outs[i]
        print(f"{case['name']:36s} blocks={len(case['blocks'])}")
    gdir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(gdir, exist_ok=True)
    np.savez_compressed(os.path.join(gdir, "golden.npz"), **out)
    with open(os.path.join(gdir, "cases.json"), "w") as f:
        json.dump(case_list, f, indent=0)
    sz = os.path.getsize(os.path.join(gdir, "golden.npz"))
    print(f"{len(case_list)} cases, {len(out)} blocks, golden.npz = {sz / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
