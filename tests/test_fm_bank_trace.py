"""
CPU: what a bank of modulated SinePE voices launches -- pinned against a recorded trace, with the stand-ins of
tests/bank_trace.py (no device).

Graphs, five voices each at 48 kHz, the measured minimums set to 4:
    fm       SinePE(frequency=TransformPE(SinePE(m_i), Affine(d_i, c_i)), amplitude=a_i)        two-operator FM
    fm-walk  ... with SINE_MOD_WALK_MIN_ROWS = 4                                                  the walk: no workspace
    bell     GainPE(fm voice, gain=AdsrTriggeredPE(PeriodicTrigger(r_i), ...))                    the bank as a level
Pull scripts (test_bank_kinds_trace's two): blocks -- four contiguous pulls of 1 024 frames, then a seek back to frame
1 024; windows -- the same with 4 096 frames and windows at the level of the mix.

    python tests/test_fm_bank_trace.py --record        writes tests/golden/fm_bank_trace.json
"""

import os

import pytest

from bank_trace import assert_matches, record_main, recorded, recorded_names, run
from test_bank_kinds_trace import SCRIPTS, _calls, _pulls

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm_bank_trace.json")
K = 5
MINIMUMS = ("SINE_MOD_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES")
KINDS = {"fm": {}, "fm-walk": {"SINE_MOD_WALK_MIN_ROWS": 4}, "bell": {}}
CASES = [f"{kind}:{pulls}" for kind in KINDS for pulls in SCRIPTS]
# [name, stream, out, out_stride, batch, n, channels, sr, params, freq, freq_stride, amp, amp_stride, phase, phase_stride,
#  state, workspace]
OUT, BATCH, N, PARAMS, FREQ, AMP, PHASE, STATE, WORKSPACE = 2, 4, 5, 8, 9, 11, 13, 15, 16


def fm_voice(pg, i):
    from pygmu2_amd.transforms import Affine
    carrier = 220.0 * 2 ** (i / 12.0)
    modulator = pg.TransformPE(pg.SinePE(carrier * 1.5), func=Affine(80.0 + 20.0 * i, carrier))
    return pg.SinePE(frequency=modulator, amplitude=0.15 + 0.01 * i)


def voices(pg, kind):
    if kind in ("fm", "fm-walk"):
        return [fm_voice(pg, i) for i in range(K)]
    if kind == "bell":
        return [pg.GainPE(fm_voice(pg, i), gain=pg.AdsrTriggeredPE(pg.PeriodicTrigger(1.0 + 0.5 * i), 0.005, 0.3, 0.0, 0.1))
                for i in range(K)]
    raise KeyError(kind)


def run_case(monkeypatch, name):
    """-> the canonical trace of case `name`."""
    import pygmu2_amd as pg
    kind, pulls = name.split(":")
    pulls, mix_windows = SCRIPTS[pulls]
    return run(monkeypatch, lambda: voices(pg, kind), pulls, switches={**{minimum: 4 for minimum in MINIMUMS}, **KINDS[kind]},
               mix_windows=mix_windows)


@pytest.mark.parametrize("name", CASES)
def test_launch_trace(monkeypatch, name):
    assert_matches(name, run_case(monkeypatch, name), recorded(FIXTURE)[name])


@pytest.mark.parametrize("pulls", list(SCRIPTS))
@pytest.mark.parametrize("kind", ["fm", "fm-walk"])
def test_an_fm_bank_is_one_call_behind_its_modulators(monkeypatch, kind, pulls):
    trace = run_case(monkeypatch, f"{kind}:{pulls}")
    rendered = 0
    for entries in _pulls(trace):
        names = [e[0] for e in entries if e[0] != "pgx_memcpy_d2d"]
        blocks = names.count("pgx_sine_stateful_bank")             # (per-voice ops: pgx_transform_bank)
        assert names == ["pgx_sine_render", "pgx_transform_bank", "pgx_sine_stateful_bank", "pgx_mix_batch"] * blocks
        rendered += blocks
    assert rendered >= 4
    calls = _calls(trace, "pgx_sine_stateful_bank")
    assert all(c[BATCH] == K and c[FREQ] is not None and c[AMP] is None and c[PHASE] is None for c in calls)
    assert all(c[FREQ + 1] == c[N] for c in calls)
    assert len({c[STATE] for c in calls}) == 1 and calls[0][STATE] is not None      # one state buffer, whatever the pull
    assert len({c[PARAMS] for c in calls}) == 1
    if pulls == "windows":
        assert any(e[5] for e in _calls(trace, "return"))          # (no phase in play: it does get windows)


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_the_walk_passes_no_workspace(monkeypatch, pulls):
    with pytest.MonkeyPatch.context() as other:
        parallel = _calls(run_case(other, f"fm:{pulls}"), "pgx_sine_stateful_bank")
    walk = _calls(run_case(monkeypatch, f"fm-walk:{pulls}"), "pgx_sine_stateful_bank")
    assert parallel and len(parallel) == len(walk)
    assert all(c[WORKSPACE] is not None for c in parallel)
    # the scratch is grown when a render is longer than any before it (a window), never shrunk: one buffer per such render
    longest, grown = 0, 0
    for c in parallel:
        if c[N] > longest:
            longest, grown = c[N], grown + 1
    assert len({c[WORKSPACE] for c in parallel}) == grown == (1 if pulls == "blocks" else 3)
    assert all(c[WORKSPACE] is None for c in walk)


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_the_bell_feeds_the_gain_above_it(monkeypatch, pulls):
    trace = run_case(monkeypatch, f"bell:{pulls}")
    calls = _calls(trace, "pgx_sine_stateful_bank")
    assert calls and len({c[STATE] for c in calls}) == 1
    assert len(_calls(trace, "pgx_adsr_triggered")) == len(_calls(trace, "pgx_periodic_trigger_bank")) == len(calls)
    # every voice block the bank writes is read by a launch behind it (the gain, or the mix that takes the gain rows)
    for entries in _pulls(trace):
        for i, e in enumerate(entries):
            if e[0] == "pgx_sine_stateful_bank":
                assert any(e[OUT] in later[2:] for later in entries[i + 1:]), e


def test_fixture_has_every_case_once():
    assert recorded_names(FIXTURE) == CASES


if __name__ == "__main__":
    record_main(FIXTURE, CASES, run_case)
