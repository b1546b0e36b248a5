"""
GPU: random graphs over every exported PE kind (tests/fuzz_graphs_all.py), HIP path against

* the reference's own renders of the fuzz corpus (tests/golden/fuzz_cases.json + fuzz.npz, oracle/gen_golden_fuzz.py):
  seeds 0..99 of test_gpu_fuzz._graph, the all-kinds generator's short / long / stream seeds, hand-written cases;
* the oracle, on the all-kinds generator's seeds in the three pull patterns of test_gpu_fuzz.py (short blocks with
  negative starts, long blocks, streams with seeks and steps back).

A graph built only from bit-exact kinds (fuzz_graphs_all.bit_exact) must match exactly; every other
graph is held to test_gpu_fuzz.py's budget: 1e-5 of peak + ABS_FLOOR, 3e-5 of peak on long blocks and streams.
"""

import json
import os

import numpy as np
import pytest

from fuzz_graphs_all import bit_exact, long_case, short_case, stream_case
from test_gpu_fuzz import (ABS_FLOOR, REL_TOL, _has_self_oscillating_ladder, _reference_is_ill_conditioned,
                           _where_the_reference_is_finite)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "fuzz_cases.json")) as _f:
    CORPUS = json.load(_f)


def assert_blocks_match(case, got, want, rel, indices=None):
    """got / want: the HIP and the expected blocks (`indices`: which of the case's blocks they are)."""
    exact = bit_exact(case["graph"])
    indices = range(len(want)) if indices is None else indices
    for i, g, w in zip(indices, got, want):
        assert g.shape == w.shape, (case["name"], i, g.shape, w.shape)
        assert np.all(np.isfinite(g)), (case["graph"], i)
        if exact:
            assert np.array_equal(g, w), (case["name"], case["graph"], i, "bit-exact graph",
                                          int(np.count_nonzero(g != w)), float(np.max(np.abs(g.astype(np.float64) - w))))
            continue
        g, w = _where_the_reference_is_finite(g, w)
        peak = float(np.max(np.abs(w))) if w.size else 0.0
        err = float(np.max(np.abs(g.astype(np.float64) - w.astype(np.float64)))) if w.size else 0.0
        assert err <= rel * peak + ABS_FLOOR, (case["name"], case["graph"], case["blocks"][max(0, i - 2):i + 1], i, err,
                                               peak)


def _skip_if_reference_ill_conditioned(case, want):
    if _has_self_oscillating_ladder(case["graph"], case["sr"]) and _reference_is_ill_conditioned(case, want):
        pytest.skip("a ladder at or above self-oscillation: the reference itself is ill-conditioned over long pulls")


@pytest.fixture(scope="module")
def corpus_npz():
    return np.load(os.path.join(GOLDEN, "fuzz.npz"))


@pytest.mark.parametrize("case", CORPUS, ids=lambda c: c["name"])
def test_hip_matches_reference_corpus(case, corpus_npz):
    from spec_build import run_case as hip_run
    long = case["name"].startswith(("all_long_", "all_stream_", "hand_"))
    want = [corpus_npz[f"{case['name']}/{i}"] for i in case["keep"]]
    if long and _has_self_oscillating_ladder(case["graph"], case["sr"]):
        from oracle.graph_eval import run_case as oracle_run
        _skip_if_reference_ill_conditioned(case, oracle_run(case))
    got = hip_run(case)
    assert_blocks_match(case, [got[i] for i in case["keep"]], want, 3 * REL_TOL if long else REL_TOL, case["keep"])


def _hip_vs_oracle(case, rel, ladder_skip):
    from oracle.graph_eval import run_case as oracle_run
    from spec_build import run_case as hip_run
    want = oracle_run(case)
    if ladder_skip:
        _skip_if_reference_ill_conditioned(case, want)
    assert_blocks_match(case, hip_run(case), want, rel)


@pytest.mark.parametrize("seed", range(int(os.environ.get("PGX_FUZZ_ALL_SEEDS", "200"))))
def test_all_kinds_short_blocks(seed):
    _hip_vs_oracle(short_case(seed), REL_TOL, ladder_skip=False)


@pytest.mark.parametrize("seed", range(int(os.environ.get("PGX_FUZZ_ALL_LONG", "16"))))
def test_all_kinds_long_blocks(seed):
    # 3e-5: resonant stages in cascade multiply what their input is off by (test_gpu_fuzz.test_random_graph_long_blocks)
    _hip_vs_oracle(long_case(seed), 3 * REL_TOL, ladder_skip=True)


@pytest.mark.parametrize("seed", range(int(os.environ.get("PGX_FUZZ_ALL_STREAMS", "16"))))
def test_all_kinds_streams(seed):
    _hip_vs_oracle(stream_case(seed), 3 * REL_TOL, ladder_skip=True)
