"""What the GPU tests of NoisePE pass to tests/fixture_harness.py: a fixture case built over pygmu2_amd, and the
family's log prefixes."""

import fixture_harness as H
import noise_oracle as P
import spec_build
from fixture_harness import assert_bits      # noqa: F401  (for the test modules)


def build_case(case):
    """-> (root PE, its NoisePEs in construction order: a "reset" op resets every one of them)."""
    return spec_build.build_case(case, (P.KIND,))


def check_case(case, npz):
    # a "peak" case is one with a SlewLimiterPE in it: it reports under that family's prefix, as it always has
    H.check_case(case, npz, build_case, tag="NOISE_ERR", peak_tag="CONTROL_ERR")
