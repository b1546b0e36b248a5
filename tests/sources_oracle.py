"""KarplusStrongPE / AnalogOscPE restatements (re-exported from oracle/sources_oracle.py, where the graph oracle uses
them too) and the builder of this family's graph format, shared by the fixture generator (tools/gen_golden_sources.py,
over the reference's classes) and the tests (over pygmu2_amd's).  tests/fixture_harness.py loads the fixture."""

from __future__ import annotations

from oracle.sources_oracle import AnalogOsc, KarplusStrong, ks_geometry  # noqa: F401  (re-exported)


def build_graph(M, spec):
    """Instantiate a JSON graph spec over the namespace M (KarplusStrongPE, AnalogOscPE, SinePE, TransformPE,
    PiecewisePE, LadderPE, LadderMode, GainPE, CropPE, DelayPE, MixPE and affine(scale, offset) -> callable)."""
    if isinstance(spec, list):
        return [build_graph(M, s) for s in spec]
    if not isinstance(spec, dict):
        return spec
    t = spec["type"]
    if t == "Affine":
        return M.TransformPE(build_graph(M, spec["source"]), func=M.affine(spec["scale"], spec["offset"]))
    args = [build_graph(M, a) for a in spec.get("args", [])]
    kwargs = {k: build_graph(M, v) for k, v in spec.get("kwargs", {}).items()}
    if t == "PiecewisePE":
        args[0] = [(int(p[0]), float(p[1])) for p in args[0]]
    if t == "LadderPE" and "mode" in kwargs:
        kwargs["mode"] = getattr(M.LadderMode, kwargs["mode"])
    return getattr(M, t)(*args, **kwargs)

