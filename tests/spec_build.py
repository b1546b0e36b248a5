"""Build a pygmu2_amd PE graph (the HIP product path) from a golden-case SPEC (see oracle/golden_cases.py for the
format): oracle/spec_builder.py's table over pygmu2_amd's flat names."""

import os
import types

import pygmu2_amd as pg
from oracle import spec_builder

KEMAR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kemar")


def namespace():
    """pygmu2_amd's classes and enums, the builder's hooks, and the hooks of the families whose fixtures have formats
    of their own: affine (tests/sources_oracle.build_graph) and wav (tests/tralfam_oracle.build_case)."""
    K = types.SimpleNamespace(**{name: getattr(pg, name) for name in dir(pg) if name[:1].isupper()})
    K.transform_func = pg.transforms.from_spec
    K.hrtf = lambda azimuth, elevation: pg.SpatialHRTF(azimuth, elevation, kemar_dir=KEMAR_DIR)
    K.affine = pg.transforms.Affine
    K.wav = lambda name: pg.WavReaderPE(os.path.join(KEMAR_DIR, name))
    return K


PG = namespace()


def build(spec, shared=None, on_make=None):
    return spec_builder.build(spec, PG, shared, on_make)


def build_case(case, kinds):
    """A fixture case's graph at the case's sample rate -> (root PE, its PEs of `kinds` in construction order)."""
    pg.set_sample_rate(case["sr"])
    made = []
    return build(case["graph"], on_make=lambda kind, pe: made.append(pe) if kind in kinds else None), made


def run_case(case):
    """Render every block of a case through a started NullRenderer graph; list of arrays."""
    pg.set_sample_rate(case["sr"])
    pe = build(case["graph"])
    r = pg.NullRenderer(sample_rate=case["sr"])
    r.set_source(pe)
    r.start()
    outs = [pe.render(int(s), int(n)).data for s, n in case["blocks"]]
    r.stop()
    return outs
