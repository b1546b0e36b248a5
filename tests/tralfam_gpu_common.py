"""Helpers shared by the GPU tests of TralfamPE, SlicePE and SetExtentPE: a fixture case built over pygmu2_amd, rendered
block by block, and the comparison the fixture prescribes for it."""

import types

import numpy as np

import pygmu2_amd as pg
import tralfam_oracle as T


def namespace():
    K = types.SimpleNamespace(ArrayPE=pg.ArrayPE, DelayPE=pg.DelayPE, LoopPE=pg.LoopPE, CropPE=pg.CropPE,
                              NoisePE=pg.NoisePE, TralfamPE=pg.TralfamPE, SlicePE=pg.SlicePE,
                              SetExtentPE=pg.SetExtentPE, ExtendMode=pg.ExtendMode)
    K.wav = lambda name: pg.WavReaderPE(T.wav_path(name))
    return K


def max_err(a, b) -> float:
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


def check_case(case, npz):
    """Device render of every block against every stored sample of the fixture, by the case's rule:
    "bits"; "peak" -- max abs error <= PEAK_BOUND * peak of the case (exact zeros for a silent case); "gain" -- per
    block max abs error <= REL_TOL * peak of the block + ABS_FLOOR.  A "sampled" case (one whole-extent render of which
    the fixture keeps the sampled frames and the peak) is compared on those frames and on its peak, and in full against
    the float64 restatement of tests/tralfam_oracle.py.  Prints the measured error before asserting."""
    pg.set_sample_rate(case["sr"])
    outs, _ = T.render_case(case, namespace(), npz)
    want = npz[case["name"]]
    got = T.stored_of(case, outs)
    assert got.shape == want.shape, (got.shape, want.shape)
    if case["compare"] == "bits":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{case['name']} differs from the fixture"
        return
    if case["compare"] == "gain":
        at = 0
        for o in outs:
            w = want[at:at + o.shape[0]]
            at += o.shape[0]
            peak = float(np.max(np.abs(w))) if w.size else 0.0
            err = max_err(o, w)
            print(f"TRALFAM_ERR {case['name']} block max_abs_err={err:.3e} peak={peak:.3e}")
            assert err <= T.REL_TOL * peak + T.ABS_FLOOR, f"{case['name']}: {err:.3e} vs peak {peak:.3e}"
        return
    assert case["compare"] == "peak"
    peak = case["peak"]
    err = max_err(got, want)
    print(f"TRALFAM_ERR {case['name']} max_abs_err={err:.3e} peak={peak:.3e} ratio={err / peak if peak else 0.0:.3e}")
    if peak == 0.0:
        assert not np.any(got), f"{case['name']}: a silent case must be exactly zero"
        return
    assert err <= T.PEAK_BOUND * peak, f"{case['name']}: {err:.3e} > {T.PEAK_BOUND * peak:.3e}"
    if case["store"] == "sampled":
        whole = outs[0]
        dev_peak = float(np.max(np.abs(whole)))
        assert abs(dev_peak - peak) <= T.PEAK_BOUND * peak, f"{case['name']}: peak {dev_peak!r} vs {peak!r}"
        restated = T.restate_case(case, npz)[0]
        err = max_err(whole, restated)
        print(f"TRALFAM_ERR {case['name']} whole render vs float64 restatement max_abs_err={err:.3e}")
        assert err <= T.PEAK_BOUND * peak, f"{case['name']} (all {whole.shape[0]} frames): {err:.3e}"
