"""GPU: seeded random graphs whose roots or inner nodes are WavetablePE / TimeWarpPE over the existing PEs, against the
reference's renders of the same graphs (tests/golden/playback.npz, tools/gen_golden_playback.py): bit for bit, except
graphs whose head positions are sums of a float64 rate that is not exact (1.1), which stay within 1e-6 of the peak."""

import pytest

from fixture_harness import load_cases
from playback_gpu_common import check_case

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("playback")
FUZZ = [c for c in CASES["cases"] if c.get("fuzz")]


def test_corpus_size():
    assert len(FUZZ) >= 40


@pytest.mark.parametrize("case", FUZZ, ids=[c["name"] for c in FUZZ])
def test_random_graph_matches_reference(case):
    check_case(case, NPZ)
