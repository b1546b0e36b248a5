"""Helpers shared by the GPU tests of SampleHoldPE / TrackHoldPE / SlewLimiterPE / FunctionGenPE: a fixture case built
over pygmu2_amd, rendered in a started NullRenderer with the case's lifecycle calls, and the comparison the fixture
prescribes for it."""

import numpy as np

import pygmu2_amd as pg
import control_oracle as P
import spec_build
from playback_gpu_common import PEAK_BOUND, bits_equal      # the one bound for re-associated float64 sums

assert PEAK_BOUND == P.PEAK_BOUND
NEW_TYPES = (pg.SampleHoldPE, pg.TrackHoldPE, pg.SlewLimiterPE, pg.FunctionGenPE)


def build_case(case):
    pg.set_sample_rate(case["sr"])
    made = []
    make = P.make_with(pg.SampleHoldPE, pg.TrackHoldPE, pg.SlewLimiterPE, pg.SlewMode, pg.FunctionGenPE)

    def make_new(kind, kw):
        made.append(make(kind, kw))
        return made[-1]

    return P.build_graph(case["graph"], spec_build.build, make_new), made


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


def report(name, got, want):
    """Prints and returns (max abs error, peak of the expected samples)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print(f"CONTROL_ERR {name} max_abs_err={err:.3e} peak={peak:.3e} ratio={err / peak if peak else float('nan'):.3e}")
    return err, peak


def assert_close(name, got, want):
    err, peak = report(name, got, want)
    assert peak > 0.0 and err <= PEAK_BOUND * peak, f"{name}: max abs error {err:.3e} > {PEAK_BOUND:g} * peak {peak:.3e}"


def assert_bits(name, got, want):
    if not bits_equal(got, want):
        d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        raise AssertionError(f"{name}: differs in {int(np.sum(d > 0))} of {d.size} samples, max {float(d.max()):.3g}, "
                             f"first at {int(np.argmax(d.reshape(-1) > 0))}")


def check_case(case, npz):
    """Device render of every stored block against the fixture, in full: bit for bit, or -- "compare": "peak" -- within
    PEAK_BOUND of the case's peak.  Prints the measured error of a "peak" case before asserting."""
    outs = render_case(case)
    flat = npz[case["name"]]
    stored = P.split_blocks(case, flat)
    if case["compare"] == "bits":
        for i, want in stored.items():
            assert_bits(f"{case['name']} block {i}", outs[i], want)
        return
    assert_close(case["name"], np.concatenate([outs[i] for i in stored]), flat)
