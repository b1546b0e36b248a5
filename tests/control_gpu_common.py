"""What the GPU tests of SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE pass to tests/fixture_harness.py:
a fixture case built over pygmu2_amd, and the family's bound and log prefix."""

import control_oracle as P
import fixture_harness as H
import spec_build
from fixture_harness import assert_bits      # noqa: F401  (for the test modules)

TAG = "CONTROL_ERR"


def build_case(case):
    """-> (root PE, the PEs of the four kinds in construction order: a "reset" op resets every one of them)."""
    return spec_build.build_case(case, P.NEW_KINDS)


def assert_close(name, got, want):
    """max abs error <= PEAK_BOUND * peak of `want`, which may not be silent."""
    H.assert_peak(name, got, want, H.PEAK_BOUND, TAG)


def check_case(case, npz):
    H.check_case(case, npz, build_case, tag=TAG)
