"""Helpers shared by the GPU tests of KarplusStrongPE / AnalogOscPE: a NullRenderer-driven render of a fixture case
(its graph built over tests/spec_build.PG) and of a PE that stays started."""

import numpy as np

import pygmu2_amd as pg
import fixture_harness as H
import spec_build
from fixture_harness import bits_equal      # noqa: F401  (for the test modules)
from sources_oracle import build_graph


def render_case(case, stored_only=True):
    pg.set_sample_rate(case["sr"])
    outs = H.render_blocks(build_graph(spec_build.PG, case["graph"]), case["sr"], case["blocks"])
    keep = H.stored_blocks(case) if stored_only else range(len(outs))
    return np.concatenate([outs[i] for i in keep])


def stream(pe, sr, blocks):
    """-> (the renderer, still started; the blocks)."""
    r = pg.NullRenderer(sample_rate=sr)
    r.set_source(pe)
    r.start()
    out = [pe.render(int(s), int(n)).data.copy() for s, n in blocks]
    return r, out
