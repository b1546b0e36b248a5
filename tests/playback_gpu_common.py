"""What the GPU tests of WavetablePE / TimeWarpPE pass to tests/fixture_harness.py: a fixture case built over
pygmu2_amd, the family's reset rule and its log prefix."""

import pygmu2_amd as pg
import fixture_harness as H
import playback_oracle as P
import spec_build


def build_case(case):
    """-> (root PE, its WavetablePEs and TimeWarpPEs in construction order)."""
    return spec_build.build_case(case, P.NEW_KINDS)


def reset_heads(made):
    """A "reset" op rewinds the TimeWarpPEs alone (a WavetablePE carries nothing)."""
    H.reset_all(m for m in made if isinstance(m, pg.TimeWarpPE))


def check_case(case, npz):
    H.check_case(case, npz, build_case, reset=reset_heads, tag="PLAYBACK_ERR")
