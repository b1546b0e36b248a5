"""What the ReversePitchEchoPE tests and the fixture generator (tools/gen_golden_reverse_echo.py) share: the SPEC kind,
built here because oracle/spec_builder.py's table does not name it, and the fixture's layout.

A case of tests/golden/reverse_echo_cases.json has "blocks" -- the blocks whose float32 samples reverse_echo.npz keeps
under the case's name, one render of the whole stretch unless the case is about gaps or lifecycle "ops" -- and
"patterns": other ways to cut the same stretch into contiguous blocks.  The reference gives every pattern's samples
equal to the one-block render's to the bit (the generator checks it), so a pattern needs no samples of its own."""

import pygmu2_amd as pg
import spec_build
from oracle import spec_builder

FAMILY = "reverse_echo"
KIND = "ReversePitchEchoPE"
NEW_KINDS = (KIND,)
TAG = "REVERSE_ECHO_ERR"


def build(spec, K, shared=None, on_make=None):
    """SPEC -> PE instance over the namespace K, with one more kind than oracle/spec_builder.py's table:
    {"pe": "ReversePitchEchoPE", "source": SPEC, "block_seconds" / "pitch_ratio" / "feedback" / "alternate_direction":
    number | SPEC, "smoothing_samples": int}, keywords as they stand.  Every such node is built here, children first,
    and stands in the graph as an instance, which the table's builder passes through as a keyword's value (so the kind
    may be the root or a keyword of another node, not an entry of an "inputs" list)."""
    shared = {} if shared is None else shared

    def resolve(node):
        if isinstance(node, list):
            return [resolve(v) for v in node]
        if not isinstance(node, dict):
            return node
        if node.get("pe") != KIND:
            return {k: resolve(v) for k, v in node.items()}
        kw = {}
        for k, v in node.items():
            if k != "pe":
                v = resolve(v)
                kw[k] = spec_builder.build(v, K, shared, on_make) if spec_builder.is_spec(v) else v
        pe = getattr(K, KIND)(**kw)
        if on_make is not None:
            on_make(KIND, pe)
        return pe

    root = resolve(spec)
    return spec_builder.build(root, K, shared, on_make) if spec_builder.is_spec(root) else root


def build_case(case):
    """-> (root PE over pygmu2_amd, its ReversePitchEchoPEs in construction order)."""
    pg.set_sample_rate(case["sr"])
    made = []
    return build(case["graph"], spec_build.PG, on_make=lambda kind, pe: made.append(pe) if kind in NEW_KINDS else None), made


def pattern_cases(case):
    """The case as stored, then one case per pattern: (id, case with that pattern's blocks)."""
    out = [(case["name"], case)]
    for name, blocks in case.get("patterns", {}).items():
        out.append((f"{case['name']}/{name}", dict(case, blocks=blocks)))
    return out
