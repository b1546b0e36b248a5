"""GPU: 30 seeded random graphs with a NoisePE in them (alone in every mode and range; as the source of the
sample-and-hold -> slew -> cutoff patch, of filters, combs and gated envelopes; mixed with other NoisePEs; under crops,
delays and holds), rendered by the reference into tests/golden/noise.npz.  NoisePE is not in the package's __all__ yet,
so the exported-PE fuzz census (tests/test_oracle_fuzz_golden.py) does not reach it; this file stands in."""

import pytest

import noise_oracle as P
from fixture_harness import load_cases
from noise_gpu_common import check_case

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("noise")
FUZZ = [c for c in CASES["cases"] if c.get("fuzz")]


def test_corpus_size():
    assert len(FUZZ) >= 30
    nodes = [n for c in FUZZ for n in P.find_nodes(P.NoiseNode(c["graph"], c["sr"]))]
    assert {n.kw["mode"] for n in nodes} == set(P.MODES)
    assert {c["compare"] for c in FUZZ} == {"bits", "peak", "fuzz"}


@pytest.mark.parametrize("case", FUZZ, ids=[c["name"] for c in FUZZ])
def test_random_graph_matches_reference(case):
    check_case(case, NPZ)
