"""CPU: KarplusStrongPE / AnalogOscPE without a GPU -- the restatement in sources_oracle.py against the reference's
fixtures (tests/golden/sources*.{json,npz}), rho_for_decay_db, the classes' host-side contract, and the C ABI entries."""

import re

import numpy as np
import pytest

import pygmu2_amd as pg
from fixture_harness import load_cases, stored_blocks
from pygmu2_amd import device, look_ahead, read_ahead
from sources_oracle import AnalogOsc, KarplusStrong

DATA, NPZ = load_cases("sources")
CASES = DATA["cases"]


def _by_kind(kind, pred=lambda c: True):
    return [c for c in CASES if c["kind"] == kind and pred(c)]


def _split(arr, blocks):
    out, i = [], 0
    for _, n in blocks:
        out.append(arr[i:i + n])
        i += n
    return out


def ks_restated(case):
    ks = KarplusStrong(case["sr"], **case["graph"]["kwargs"])
    outs = [ks.render(int(s), int(n)) for s, n in case["blocks"]]
    return np.concatenate([outs[i] for i in stored_blocks(case)])


def osc_restated(case, want_edges=False):
    kw = case["graph"]["kwargs"]
    wave = kw.get("waveform", "rectangle")
    pure = not any(isinstance(kw.get(k), dict) for k in ("frequency", "duty_cycle"))
    osc = AnalogOsc(case["sr"], wave, pure)
    params = {}
    for key, name in (("frequency", "freq"), ("duty_cycle", "duty")):
        v = kw.get(key, 440.0 if key == "frequency" else 0.5)
        if isinstance(v, dict):
            params[key] = [a.astype(np.float64) for a in _split(NPZ[f"{case['name']}/{name}"], case["blocks"])]
        else:
            params[key] = [np.full(n, float(v)) for _, n in case["blocks"]]
    outs, edge = [], np.inf
    for b, (s, n) in enumerate(case["blocks"]):
        y = osc.render(int(s), params["frequency"][b], params["duty_cycle"][b]).astype(np.float32)
        outs.append(np.repeat(y[:, None], kw.get("channels", 1), axis=1))
        if not pure:
            edge = min(edge, osc.edge_distance())
    out = np.concatenate([outs[i] for i in stored_blocks(case)])
    return (out, edge, pure) if want_edges else out


@pytest.mark.parametrize("case", _by_kind("ks"), ids=lambda c: c["name"])
def test_ks_restatement_bit_exact(case):
    got = ks_restated(case)
    want = NPZ[case["name"]]
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", _by_kind("osc"), ids=lambda c: c["name"])
def test_osc_restatement(case):
    got, edge, pure = osc_restated(case, want_edges=True)
    want = NPZ[case["name"]]
    assert got.shape == want.shape
    if pure and case["graph"]["kwargs"]["waveform"] == "rectangle":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        peak = float(np.max(np.abs(want)))
        assert float(np.max(np.abs(got.astype(np.float64) - want))) <= 1e-6 * peak
    if not pure:
        assert edge > 1e-9, edge          # no phase near a discontinuity: the device comparison is total


def test_rho_for_decay_db_matches_reference():
    for seconds, f, sr, db, rho in NPZ["rho/grid"]:
        assert pg.rho_for_decay_db(seconds, f, int(sr), db=db) == rho
    for seconds, f, sr, msg in DATA["rho_errors"]:
        with pytest.raises(ValueError, match=re.escape(msg)):
            pg.rho_for_decay_db(seconds, f, sr)


def test_karplus_strong_contract():
    pg.set_sample_rate(44100)
    for kw, msg in (({"frequency": 0}, "frequency must be positive"), ({"frequency": 440, "rho": 0}, "rho must be"),
                    ({"frequency": 440, "rho": 1.5}, "rho must be"), ({"frequency": 440, "amplitude": 0}, "amplitude"),
                    ({"frequency": 440, "duration": -1, "rho_damping": 0.9}, "duration must be >= 0"),
                    ({"frequency": 440, "duration": 10, "rho_damping": 0.0}, "rho_damping must be")):
        with pytest.raises(ValueError, match=msg):
            pg.KarplusStrongPE(**kw)
    ks = pg.KarplusStrongPE(440.0, rho=0.99, duration=100, rho_damping=0.9, channels=2)
    assert repr(ks) == "KarplusStrongPE(frequency=440.0, rho=0.99, duration=100, rho_damping=0.9)"
    assert repr(pg.KarplusStrongPE(220, duration=5)) == "KarplusStrongPE(frequency=220.0, rho=0.996)"
    assert not ks.is_pure() and ks.inputs() == [] and ks.channel_count() == 2
    assert (ks.extent().start, ks.extent().end) == (0, None)
    assert look_ahead.capable(ks) and not read_ahead.eligible(ks)


def test_analog_osc_contract():
    pg.set_sample_rate(44100)
    with pytest.raises(ValueError, match="waveform must be"):
        pg.AnalogOscPE(waveform="square")
    with pytest.raises(ValueError, match="channels must be >= 1"):
        pg.AnalogOscPE(channels=0)
    rect = pg.AnalogOscPE(110.0, 0.3, "Rectangle", channels=2)
    saw = pg.AnalogOscPE(110.0, 0.3, "sawtooth")
    assert rect.waveform == "rectangle" and rect.channel_count() == 2 and rect.is_pure()
    assert repr(rect) == "AnalogOscPE(frequency=110.0, duty_cycle=0.3, waveform='rectangle', channels=2)"
    assert (rect.extent().start, rect.extent().end) == (None, None)
    sweep = pg.PiecewisePE([(0, 100.0), (5000, 200.0)])
    st = pg.AnalogOscPE(frequency=sweep, duty_cycle=0.5, waveform="sawtooth")
    assert not st.is_pure() and st.inputs() == [sweep]
    assert repr(st) == "AnalogOscPE(frequency=PiecewisePE, duty_cycle=0.5, waveform='sawtooth', channels=1)"
    assert st.extent() == sweep.extent()
    # a pure sawtooth integrates within each request: no read-ahead window, no look-ahead window
    assert read_ahead.eligible(rect)
    assert not read_ahead.eligible(saw) and not look_ahead.capable(saw)
    assert look_ahead.capable(st)
    st_rect = pg.AnalogOscPE(frequency=110.0, duty_cycle=pg.PiecewisePE([(0, 0.2), (5000, 0.8)]))
    assert look_ahead.capable(st_rect)


def test_abi_covers_new_entries():
    names = ("pgx_karplus_strong", "pgx_analog_osc_workspace_bytes", "pgx_analog_osc_pure", "pgx_analog_osc_stateful")
    for name in names:
        assert name in device._ABI.functions, name
        assert name in device.EXPORTED_SYMBOLS
    assert device.KS_PARAMS.itemsize == 40 and device.KS_STATE.itemsize == 16
    lib = device.load_library()
    for name in names:
        assert hasattr(lib, name)
    assert lib.pgx_analog_osc_workspace_bytes(0) == 0
    assert lib.pgx_analog_osc_workspace_bytes(2048) == 2 * (2 + 4) * 8
