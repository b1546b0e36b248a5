"""GPU: the graphs of the reference's examples/21_analog_osc.py and examples/29_karplus_strong.py against the
reference's renders (1024-frame blocks; the fixture keeps every 8th block).  The KarplusStrongPE graphs are bit-exact
(CropPE / DelayPE / MixPE add no rounding of their own).  The AnalogOscPE graphs run at the examples' 110 / 220 Hz,
where the float64 phase passes within rounding of a whole cycle every 4 410 / 2 205 frames: the device's prefix sum
and numpy's cumsum may then land on the two sides of the wrap, so those graphs are held to
1e-6 of peak up to the first such frame; after it the sawtooth graph is compared between whole-cycle frames up to its
constant shift (1e-5 of peak), the rectangle graphs by their audible shape (correlation)."""

import numpy as np
import pytest

from fixture_harness import load_cases, stored_blocks
from sources_gpu_common import bits_equal, render_case

pytestmark = pytest.mark.gpu

DATA, NPZ = load_cases("sources")
EXAMPLES = [c for c in DATA["cases"] if c["kind"] == "example"]
FIRST_WRAP = {"ex21_pwm": 4410, "ex21_morph": 2205, "ex21_subtractive": 4410}


@pytest.mark.parametrize("case", EXAMPLES, ids=lambda c: c["name"])
def test_example_graph(case):
    got = render_case(case)
    want = NPZ[case["name"]]
    assert got.shape == want.shape
    if case["name"].startswith("ex29"):
        assert bits_equal(got, want)
        return
    head = FIRST_WRAP[case["name"]]              # stored block 0 is frames 0 .. 1023, block 1 is 8192 .. 9215
    peak = float(np.max(np.abs(want)))
    err = np.abs(got.astype(np.float64) - want)
    assert np.max(err[:min(head, 1024)]) <= 1e-6 * peak
    if case["name"] == "ex21_morph":
        blocks = case["blocks"]
        frames = np.concatenate([np.arange(blocks[i][0], blocks[i][0] + blocks[i][1]) for i in stored_blocks(case)])
        seg = (frames - 1) // head                   # a flip at a whole-cycle frame shifts the integral after it
        d = got[:, 0].astype(np.float64) - want[:, 0]
        for k in np.unique(seg):
            dk = d[seg == k]
            assert np.max(np.abs(dk - dk.mean())) <= 1e-5 * peak, k
        return
    corr = float(np.corrcoef(got[:, 0], want[:, 0])[0, 1])
    assert corr > 0.99, corr
