"""GPU: 40 seeded random graphs mixing SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE with existing PEs
(holds of noise, sines and generator output under triggers, gates and +-1 rectangles; slew limiters over them; the
result as a gain, behind a delay, under a crop, as a filter cutoff), rendered by the reference into
tests/golden/control.npz.  The four classes are not in the package's __all__ yet, so the exported-PE fuzz census
(tests/test_oracle_fuzz_golden.py) does not reach them; this file stands in."""

import pytest

import control_oracle as P
from control_gpu_common import check_case
from fixture_harness import load_cases

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("control")
FUZZ = [c for c in CASES["cases"] if c.get("fuzz")]


def test_corpus_size():
    assert len(FUZZ) >= 40
    kinds = {n.kind for c in FUZZ for n in P.find_nodes(P.ControlNode(c["graph"], c["sr"]), P.NEW_KINDS)}
    assert kinds == set(P.NEW_KINDS)


@pytest.mark.parametrize("case", FUZZ, ids=[c["name"] for c in FUZZ])
def test_random_graph_matches_reference(case):
    check_case(case, NPZ)
