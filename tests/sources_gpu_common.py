"""Helpers shared by the GPU tests of KarplusStrongPE / AnalogOscPE: the graph namespace over pygmu2_amd and a
NullRenderer-driven render of a fixture case."""

import types

import numpy as np

import pygmu2_amd as pg
from sources_oracle import build_graph, stored_blocks

PG = types.SimpleNamespace(
    KarplusStrongPE=pg.KarplusStrongPE, AnalogOscPE=pg.AnalogOscPE, SinePE=pg.SinePE, TransformPE=pg.TransformPE,
    PiecewisePE=pg.PiecewisePE, LadderPE=pg.LadderPE, LadderMode=pg.LadderMode, GainPE=pg.GainPE, CropPE=pg.CropPE,
    DelayPE=pg.DelayPE, MixPE=pg.MixPE, affine=lambda scale, offset: pg.transforms.Affine(scale, offset))


def render_case(case, stored_only=True):
    pg.set_sample_rate(case["sr"])
    pe = build_graph(PG, case["graph"])
    r = pg.NullRenderer(sample_rate=case["sr"])
    r.set_source(pe)
    r.start()
    outs = [pe.render(int(s), int(n)).data.copy() for s, n in case["blocks"]]
    r.stop()
    keep = stored_blocks(case) if stored_only else range(len(outs))
    return np.concatenate([outs[i] for i in keep])


def stream(pe, sr, blocks):
    r = pg.NullRenderer(sample_rate=sr)
    r.set_source(pe)
    r.start()
    out = [pe.render(int(s), int(n)).data.copy() for s, n in blocks]
    return r, out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
