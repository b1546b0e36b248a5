"""Helpers shared by the GPU tests of WavetablePE / TimeWarpPE: a fixture case built over pygmu2_amd, rendered in a
started NullRenderer with the case's lifecycle calls, and the comparison the fixture prescribes for it."""

import numpy as np

import pygmu2_amd as pg
import playback_oracle as P
import spec_build

PEAK_BOUND = 1e-6          # re-associated float64 sums: max abs error <= 1e-6 * peak of the case


def build_case(case):
    pg.set_sample_rate(case["sr"])
    made = []
    make = P.make_with(pg.WavetablePE, pg.TimeWarpPE, pg.InterpolationMode, pg.OutOfBoundsMode)

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
                if isinstance(m, pg.TimeWarpPE):
                    m.reset_state()
        outs.append(pe.render(int(s), int(n)).data.copy())
    r.stop()
    return outs


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_case(case, npz):
    """Device render of every stored block against the fixture, in full: bit for bit, or -- "compare": "peak" -- within
    PEAK_BOUND of the case's peak.  Prints the measured error of a "peak" case before asserting."""
    outs = render_case(case)
    flat = npz[case["name"]]
    stored = P.split_blocks(case, flat)
    if case["compare"] == "bits":
        for i, want in stored.items():
            if not bits_equal(outs[i], want):
                d = np.abs(outs[i].astype(np.float64) - want.astype(np.float64))
                raise AssertionError(f"{case['name']}: block {i} differs from the reference in {int(np.sum(d > 0))} of "
                                     f"{d.size} samples, max {float(d.max()):.3g}, first at {int(np.argmax(d > 0))}")
        return 0.0
    peak = float(np.max(np.abs(flat)))
    err = max(float(np.max(np.abs(outs[i].astype(np.float64) - want.astype(np.float64)))) for i, want in stored.items())
    print(f"PLAYBACK_ERR {case['name']} max_abs_err={err:.3e} peak={peak:.3e} ratio={err / peak:.3e}")
    assert all(outs[i].shape == want.shape for i, want in stored.items())
    assert err <= PEAK_BOUND * peak, f"{case['name']}: max abs error {err:.3e} > {PEAK_BOUND:g} * peak {peak:.3e}"
    return err
