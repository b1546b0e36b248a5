"""
CPU: the oracle against the reference at 3, 4, 5 and 8 channels -- tests/golden/channels_cases.json + channels.npz,
rendered by the reference's own classes (tools/gen_golden_channels.py) from the cases of tests/channel_cases.py -- by the
rule tests/test_oracle_fuzz_golden.py applies to its corpus.  The GPU tests (tests/test_gpu_channels.py) judge the
kernels by this oracle on the blocks the fixture does not store; this pins the oracle there first.

And the comparison against itself: a stored block with two columns swapped, or with one column a frame late, must be
rejected, by this module's rule and by the one the GPU test applies (channel_cases.compare_block) -- a case that
accepted either would have too symmetric an input to notice a wrong channel index.
"""

import json
import os

import numpy as np
import pytest

import channel_cases
from fuzz_graphs_all import kinds, osc_edge_distance
from test_oracle_fuzz_golden import NOT_BIT_EXACT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "channels_cases.json")) as _f:
    CASES = json.load(_f)
PROCESSORS = [c for c in CASES if not channel_cases.is_source_case(c)]
SOURCES = [c for c in CASES if channel_cases.is_source_case(c)]


@pytest.fixture(scope="module")
def npz():
    return np.load(os.path.join(GOLDEN, "channels.npz"))


def oracle_mismatch(case, i, got, want):
    """None when `got` reproduces the reference's block `want` by test_oracle_fuzz_golden.py's rule (bit for bit; a
    graph that holds a NOT_BIT_EXACT kind within that kind's bound of the block's peak), else what is wrong."""
    loose = [NOT_BIT_EXACT[k] for k in kinds(case["graph"]) if k in NOT_BIT_EXACT]
    if got.dtype != np.float32 or got.shape != want.shape:
        return f"{case['name']} block {i}: {got.dtype} {got.shape}, the reference has float32 {want.shape}"
    if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return None
    if not loose:
        return f"{case['name']} block {i}: not bit for bit, max {float(np.max(np.abs(got.astype(np.float64) - want))):.3e}"
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return f"{case['name']} block {i}: NaNs elsewhere"
    ok = np.isfinite(want)
    peak = float(np.max(np.abs(want[ok]))) if ok.any() else 0.0
    err = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) if ok.any() else 0.0
    return None if err <= max(loose) * peak else f"{case['name']} block {i}: {err:.3e} > {max(loose):g} * {peak:.3e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle_reproduces_reference_at_many_channels(case, npz):
    from oracle.graph_eval import run_case
    outs = run_case(case)
    for (_, n), out in zip(case["blocks"], outs):
        assert out.shape[0] == n and out.shape[1] >= 2, (case["name"], out.shape)
    for i in case["keep"]:
        wrong = oracle_mismatch(case, i, outs[i], npz[f"{case['name']}/{i}"])
        assert wrong is None, wrong


def _swapped(block):
    out = block.copy()
    out[:, [0, 1]] = block[:, [1, 0]]
    return out


def _late(block):
    out = block.copy()
    out[1:, 0] = block[:-1, 0]
    return out


@pytest.mark.parametrize("case", PROCESSORS, ids=lambda c: c["name"])
def test_comparison_rejects_swapped_and_late_columns(case, npz):
    stored = {i: npz[f"{case['name']}/{i}"] for i in case["keep"]}
    for i, want in stored.items():                    # the expectation itself passes both rules
        assert oracle_mismatch(case, i, want.copy(), want) is None
        assert channel_cases.compare_block(case, i, want.copy(), want)[0]
    for what, mutate in (("columns 0 and 1 swapped", _swapped), ("column 0 a frame late", _late)):
        by_oracle_rule = [oracle_mismatch(case, i, mutate(w), w) is not None for i, w in stored.items()]
        by_gpu_rule = [not channel_cases.compare_block(case, i, mutate(w), w)[0] for i, w in stored.items()]
        assert any(by_oracle_rule) and any(by_gpu_rule), (case["name"], what, "accepted: the input is too symmetric")


@pytest.mark.parametrize("case", SOURCES, ids=lambda c: c["name"])
def test_source_cases_tile_one_column(case, npz):
    """A source built with channels=C repeats one column (no swap can show there): every stored column is the first,
    and the case has as many columns as it asked for."""
    for i in case["keep"]:
        want = npz[f"{case['name']}/{i}"]
        assert want.shape[1] == case["C"], (case["name"], want.shape)
        assert np.array_equal(want, np.repeat(want[:, :1], want.shape[1], axis=1)), (case["name"], i)


def test_fixture_is_what_channel_cases_lists():
    """The stored specs are channel_cases.cases() (a change there means rendering the fixture again), every PE kind has
    its channel counts, no stateful oscillator sits on a waveform edge, and the two files stay within 1 MB."""
    listed = channel_cases.cases()
    assert [{k: v for k, v in c.items() if k != "keep"} for c in CASES] == json.loads(json.dumps(listed))
    by_kind = {}
    for c in CASES:
        by_kind.setdefault(c["kind"], set()).add(c["C"])
    chain = {"BiquadPE", "SVFilterPE", "CombPE", "EnvelopePE", "LadderPE", "KarplusStrongPE", "CompressorPE", "LimiterPE",
             "ExpanderPE", "DynamicsPE"}
    for kind, counts in by_kind.items():
        want = channel_cases.CHAIN_C if kind in chain else channel_cases.ELEMENTWISE_C
        assert set(want) <= counts, (kind, sorted(counts))
    for c in CASES:
        if "AnalogOscPE" in kinds(c["graph"]):
            assert osc_edge_distance(c) > 1e-9, c["name"]
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("channels_cases.json", "channels.npz"))
    assert total <= 1_000_000, total
