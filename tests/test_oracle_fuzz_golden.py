"""
CPU: the oracle against the reference on random graphs -- tests/golden/fuzz_cases.json + fuzz.npz, rendered by the
reference's own classes (oracle/gen_golden_fuzz.py): seeds 0..99 of test_gpu_fuzz._graph, seeds of the all-kinds
generator (tests/fuzz_graphs_all.py) in short blocks, long blocks and streams, and hand-written interaction cases.
The GPU fuzz compares the HIP path with the oracle; this pins the oracle itself on the same kind of graphs.
"""

import json
import os

import numpy as np
import pytest

import pygmu2_amd as pg
from fuzz_graphs_all import kinds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "fuzz_cases.json")) as _f:
    CASES = json.load(_f)

# The only stored blocks the oracle does not reproduce bit for bit, by the kind that explains them, with the bound
# asserted.  LadderPE: the oracle runs the reference's numba kernel as a C restatement (oracle/seq_kernels.c), whose
# tanh / division roundings can differ from numpy's in the last bit, and the feedback carries that on -- measured on
# this corpus: one block (fuzz_37), 7.1e-12 of its peak.
NOT_BIT_EXACT = {"LadderPE": 1e-6}

# Exported PE classes the corpus need not contain, with why.
NOT_FUZZED = {
    "SourcePE": "an abstract base class: nothing to render",
    "GateSignal": "an abstract base class (PeriodicGate is its fuzzed subclass)",
    "TriggerSignal": "an abstract base class (PeriodicTrigger is its fuzzed subclass)",
    "WavReaderPE": "reads a file: WAV I/O has its own tests (tests/test_wav_io.py) and is out of the fuzz's scope",
    "WavWriterPE": "writes a file (a pass-through for its source's samples): WAV I/O, as above",
}
MIN_CASES = 5


@pytest.fixture(scope="module")
def npz():
    return np.load(os.path.join(GOLDEN, "fuzz.npz"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle_reproduces_reference_on_random_graphs(case, npz):
    from oracle.graph_eval import run_case
    outs = run_case(case)
    loose = [NOT_BIT_EXACT[k] for k in kinds(case["graph"]) if k in NOT_BIT_EXACT]
    for i in case["keep"]:
        want, got = npz[f"{case['name']}/{i}"], outs[i]
        assert got.dtype == np.float32 and got.shape == want.shape, (case["name"], i, got.shape, want.shape)
        if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            continue
        assert loose, (case["name"], i, "not bit for bit", float(np.max(np.abs(got.astype(np.float64) - want))))
        assert np.array_equal(np.isnan(got), np.isnan(want)), (case["name"], i)
        ok = np.isfinite(want)
        peak = float(np.max(np.abs(want[ok]))) if ok.any() else 0.0
        err = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) if ok.any() else 0.0
        assert err <= max(loose) * peak, (case["name"], i, err, peak)


def test_every_exported_pe_is_fuzzed():
    """Every PE class in pygmu2_amd.__all__ appears in at least MIN_CASES corpus cases, bar NOT_FUZZED: a PE added
    later without fuzz coverage fails here."""
    import inspect
    exported = sorted(n for n in pg.__all__ if n != "ProcessingElement"
                      and inspect.isclass(getattr(pg, n)) and issubclass(getattr(pg, n), pg.ProcessingElement))
    assert "KarplusStrongPE" in exported and "CachePE" in exported and "PeriodicGate" in exported
    count = {n: 0 for n in exported}
    for case in CASES:
        for k in kinds(case["graph"]):
            if k in count:
                count[k] += 1
    missing = {n: c for n, c in count.items() if c < MIN_CASES and n not in NOT_FUZZED}
    assert not missing, missing
    assert set(NOT_FUZZED) <= set(exported)


def test_corpus_is_what_the_generators_draw():
    """The stored specs are the generators' current draws: a change to a generator (or to test_gpu_fuzz._graph, whose
    seeds must keep their graphs) shows up here, and the corpus must then be rendered again."""
    import fuzz_graphs_all as F
    import test_gpu_fuzz
    by_name = {c["name"]: c for c in CASES}
    for seed in (0, 1, 37, 99):
        want = test_gpu_fuzz._graph(seed)
        assert by_name[want["name"]]["graph"] == want["graph"] and by_name[want["name"]]["blocks"] == want["blocks"]
    for seed in (0, 1, 77, 149):
        want = F.short_case(seed)
        assert by_name[want["name"]]["graph"] == want["graph"] and by_name[want["name"]]["blocks"] == want["blocks"]
    assert sum(1 for c in CASES if c["name"].startswith("hand_")) >= 10


def test_corpus_size():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("fuzz_cases.json", "fuzz.npz"))
    assert total <= 2_000_000, total
