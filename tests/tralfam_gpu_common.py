"""What the GPU tests of TralfamPE, SlicePE and SetExtentPE add to tests/fixture_harness.py: a fixture case of this
family's format built over pygmu2_amd and rendered block by block, its rule for a silent case, and the two extra checks
of a "sampled" case."""

import numpy as np

import pygmu2_amd as pg
import fixture_harness as H
import spec_build
import tralfam_oracle as T

TAG = "TRALFAM_ERR"


def check_case(case, npz):
    """Device render of every block against every stored sample of the fixture, by the case's rule: "bits"; "peak" --
    max abs error <= PEAK_BOUND * the fixture's peak of the case (exact zeros for a silent case); "gain" -- per block max
    abs error <= REL_TOL * peak of the block + ABS_FLOOR.  A "sampled" case (one whole-extent render of which the
    fixture keeps the sampled frames and the peak) is compared on those frames and on its peak, and in full against the
    float64 restatement of tests/tralfam_oracle.py.  Prints the measured error before asserting."""
    pg.set_sample_rate(case["sr"])
    outs, _ = T.render_case(case, spec_build.PG, npz)
    want = npz[case["name"]]
    if case["compare"] == "gain":
        stored = H.split_blocks({"name": case["name"], "blocks": [[0, o.shape[0]] for o in outs]}, want)
        H.assert_per_block(case["name"], outs, stored, H.REL_TOL, H.ABS_FLOOR, TAG, numbered=False)
        return
    got = T.stored_of(case, outs)
    if case["compare"] == "bits":
        H.assert_bits(case["name"], got, want)
        return
    assert case["compare"] == "peak"
    peak = case["peak"]
    H.assert_peak(case["name"], got, want, H.PEAK_BOUND, TAG, silent="zero", peak=peak)
    if peak > 0.0 and case["store"] == "sampled":
        whole = outs[0]
        dev_peak = float(np.max(np.abs(whole)))
        assert abs(dev_peak - peak) <= H.PEAK_BOUND * peak, f"{case['name']}: peak {dev_peak!r} vs {peak!r}"
        restated = T.restate_case(case, npz)[0]
        err = H.max_err(whole, restated)
        print(f"{TAG} {case['name']} whole render vs float64 restatement max_abs_err={err:.3e}")
        assert err <= H.PEAK_BOUND * peak, f"{case['name']} (all {whole.shape[0]} frames): {err:.3e}"
