"""Helpers shared by the GPU tests of NoisePE: a fixture case built over pygmu2_amd, rendered in a started NullRenderer
with the case's lifecycle calls, and the comparison the fixture prescribes for it."""

import numpy as np

import pygmu2_amd as pg
import control_oracle as C
import noise_oracle as P
import spec_build
from control_gpu_common import assert_bits, assert_close      # noqa: F401  (bit equality / PEAK_BOUND of the case's peak)


def build_case(case):
    pg.set_sample_rate(case["sr"])
    made = []
    make = P.make_with(pg.NoisePE, pg.NoiseMode,
                       C.make_with(pg.SampleHoldPE, pg.TrackHoldPE, pg.SlewLimiterPE, pg.SlewMode, pg.FunctionGenPE))

    def make_new(kind, kw):
        pe = make(kind, kw)
        if kind == P.KIND:
            made.append(pe)
        return pe

    return P.build_graph(case["graph"], spec_build.build, make_new, lambda inputs: pg.MixPE(*inputs)), made


def render_case(case):
    """Every block of the case, in order -> list of arrays."""
    pe, made = build_case(case)
    r = pg.NullRenderer(sample_rate=case["sr"])
    r.set_source(pe)
    r.start()
    ops = {int(k): v for k, v in case.get("ops", {}).items()}
    outs = []
    for i, (s, n) in enumerate(case["blocks"]):
        if ops.get(i) == "restart":
            r.stop()
            r.start()
        elif ops.get(i) == "reset":
            for m in made:
                m.reset_state()
        outs.append(pe.render(int(s), int(n)).data.copy())
    r.stop()
    return outs


def check_case(case, npz):
    """Device render of every stored block against the fixture, in full, by the case's rule: "bits"; "peak" -- max abs
    error <= PEAK_BOUND * peak of the case; "fuzz" -- per block max abs error <= REL_TOL * peak of the block +
    ABS_FLOOR.  Prints the measured error of a case that is not compared to the bit before asserting."""
    outs = render_case(case)
    flat = npz[case["name"]]
    stored = P.split_blocks(case, flat)
    assert stored
    if case["compare"] == "bits":
        for i, want in stored.items():
            assert_bits(f"{case['name']} block {i}", outs[i], want)
        return
    if case["compare"] == "peak":
        assert_close(case["name"], np.concatenate([outs[i] for i in stored]), flat)
        return
    assert case["compare"] == "fuzz"
    for i, want in stored.items():
        assert outs[i].shape == want.shape
        peak = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(outs[i].astype(np.float64) - want.astype(np.float64))))
        print(f"NOISE_ERR {case['name']} block {i} max_abs_err={err:.3e} peak={peak:.3e}")
        assert err <= P.REL_TOL * peak + P.ABS_FLOOR, f"{case['name']} block {i}: {err:.3e} vs peak {peak:.3e}"
