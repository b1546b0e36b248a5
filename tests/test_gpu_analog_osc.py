"""GPU: AnalogOscPE (pgx_analog_osc_pure / pgx_analog_osc_stateful) against the reference's fixtures and the float64
restatement: the pure rectangle bit for bit, the integrating forms to 1e-6 of peak; the pure sawtooth's dependence on
how a stream is cut into requests is the reference's; look-ahead windows leave the stateful form's samples unchanged."""

import numpy as np
import pytest

import pygmu2_amd as pg
from fixture_harness import load_cases
from pygmu2_amd import look_ahead
from sources_gpu_common import bits_equal, render_case, stream
from sources_oracle import AnalogOsc

pytestmark = pytest.mark.gpu

DATA, NPZ = load_cases("sources")
OSC_CASES = [c for c in DATA["cases"] if c["kind"] == "osc"]
SR = 44100


def _is_pure_rect(case):
    kw = case["graph"]["kwargs"]
    return kw.get("waveform") == "rectangle" and not any(isinstance(v, dict) for v in kw.values())


@pytest.mark.parametrize("case", OSC_CASES, ids=lambda c: c["name"])
def test_goldens(case):
    got = render_case(case)
    want = NPZ[case["name"]]
    assert got.shape == want.shape
    if _is_pure_rect(case):
        assert bits_equal(got, want)
    else:
        # (tests/test_sources_host.py asserts that no restated phase of these cases lies within 1e-9 of an edge)
        peak = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(got.astype(np.float64) - want))) <= 1e-6 * peak


def test_pure_rectangle_long_and_far():
    pg.set_sample_rate(SR)
    for f, d, start in ((110.0, 0.3, 0), (3520.7, 0.5, 123_456_789), (12000.0, 0.1, -(1 << 22))):
        n = 1 << 20
        got = pg.AnalogOscPE(f, d).render(start, n).data[:, 0]
        want = AnalogOsc(SR, "rectangle", True).render(start, np.full(n, f), np.full(n, d)).astype(np.float32)
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert int(ulp.max()) <= 1, (f, d, start)


def test_pure_sawtooth_depends_on_requests_like_the_reference():
    pg.set_sample_rate(SR)
    f, d, n, block = 110.0, 0.3, 64 * 1024, 1024
    pe = pg.AnalogOscPE(f, d, "sawtooth")
    one = pe.render(0, n).data[:, 0]
    blocks = np.concatenate([pe.render(s, block).data[:, 0] for s in range(0, n, block)])
    ref = AnalogOsc(SR, "sawtooth", True)
    want_one = ref.render(0, np.full(n, f), np.full(n, d))
    want_blocks = np.concatenate([ref.render(s, np.full(block, f), np.full(block, d)) for s in range(0, n, block)])
    peak = float(np.max(np.abs(want_one)))
    assert np.max(np.abs(one - want_one)) <= 1e-6 * peak
    assert np.max(np.abs(blocks - want_blocks)) <= 1e-6 * np.max(np.abs(want_blocks))
    assert np.max(np.abs(want_one - want_blocks)) > 1e-3          # the partition dependence is real ...
    assert np.max(np.abs(one - blocks)) > 1e-3                    # ... and reproduced
    assert not look_ahead.capable(pe)


def _stateful_graph():
    freq = pg.PiecewisePE([(0, 80.3), (1 << 20, 5000.0)])
    duty = pg.TransformPE(pg.SinePE(frequency=0.7), func=pg.transforms.Affine(0.4, 0.5))
    return freq, duty


def test_stateful_2_20_frames():
    pg.set_sample_rate(SR)
    n = 1 << 20
    for wave in ("rectangle", "sawtooth"):
        freq, duty = _stateful_graph()
        pe = pg.AnalogOscPE(freq, duty, wave)
        _, out = stream(pe, SR, [(0, n)])
        got = out[0][:, 0].astype(np.float64)
        fv = freq.render(0, n).data[:, 0].astype(np.float64)
        dv = duty.render(0, n).data[:, 0].astype(np.float64)
        osc = AnalogOsc(SR, wave, False)
        want = osc.render(0, fv, dv)
        e = (1.0 - osc.duties) if wave == "sawtooth" else osc.duties
        near = np.minimum(np.minimum(np.abs(osc.phases - e), osc.phases), 1.0 - osc.phases) < 1e-9
        near[0] = False
        assert int(near.sum()) == 0, (wave, int(near.sum()))
        peak = float(np.max(np.abs(want)))
        assert np.max(np.abs(got - want)) <= 1e-5 * peak, wave


def _la_run(enabled, wave):
    look_ahead.set_enabled(enabled)
    try:
        pg.set_sample_rate(SR)
        freq, duty = _stateful_graph()
        pe = pg.AnalogOscPE(freq, duty, wave)
        if enabled:
            assert look_ahead.capable(pe)
        blocks = [(s, 1024) for s in range(0, 80 * 1024, 1024)] + [(300_000, 1024)] + \
                 [(s, 1024) for s in range(301_024, 301_024 + 30 * 1024, 1024)]
        r, out = stream(pe, SR, blocks)
        pe.reset_state()
        out += [pe.render(s, 1024).data.copy() for s in range(0, 20 * 1024, 1024)]
        look_ahead.before_direct_access(pe)
        state = pe._state.to_host().copy()
        r.stop()
        return out, state
    finally:
        look_ahead.set_enabled(True)


@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
def test_look_ahead_matches_block_by_block(wave):
    a, sa = _la_run(True, wave)
    b, sb = _la_run(False, wave)
    for x, y in zip(a, b):
        assert np.max(np.abs(x.astype(np.float64) - y)) <= 1e-6 * max(1.0, float(np.max(np.abs(y))))
    assert np.allclose(sa, sb, rtol=0, atol=1e-9)
