"""
CPU: the kinds of bank and the paths of voice_bank.py that the other trace tests leave out -- pinned against a recorded
trace, with the stand-ins of tests/bank_trace.py (no device).

Graphs, five voices each at 48 kHz, the measured minimums set to 4:
    pwm                  AnalogOscPE(f_i, duty_cycle=TransformPE(SinePE(r_i), Affine(0.4, 0.5)), "rectangle")   stateful
    saw-pure             AnalogOscPE(f_i, waveform="sawtooth")                       request-dependent: never a window
    adapter              SpatialPE(SinePE(f_i), SpatialAdapter(2))                   _AdaptNode
    transform-per-voice  TransformPE(SinePE(r_i), Affine(300, 100 i))                per-voice ops: pgx_transform_bank
    svf                  SVFilterPE(BlitSawPE(f_i), 1000 + i, 2, LOWPASS)            the segmented plan (a workspace)
    svf-walk             ... with SVF_WALK_MIN_ROWS = 4                              the walk: no workspace
    swept-walk           test_noise_bank_trace's swept voice, BIQUAD_VAR_WALK_MIN_ROWS = 4                the walk
    sine-gate            GainPE(SinePE(f_i), gain=AdsrGatedPE(SinePE(2 + i), ...))   a gate that is no PeriodicGate
    stereo-biquad        BiquadPE(SinePE(f_i, channels=2), 1000, 0.7)                pgx_biquad_const, two channels
    stereo-ladder        LadderPE(SinePE(f_i, channels=2), 1000 + 50 i, 0.3)         pgx_ladder, two channels
Pull scripts: blocks -- four contiguous pulls of 1 024 frames, then a seek back to frame 1 024; windows -- the same with
4 096 frames and windows at the level of the mix.

    python tests/test_bank_kinds_trace.py --record        writes tests/golden/bank_kinds_trace.json
"""

import os

import pytest

from bank_trace import assert_matches, install, record_main, recorded, recorded_names, run

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bank_kinds_trace.json")
K = 5
MINIMUMS = ("ANALOG_OSC_MIN_VOICES", "NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES",
            "BIQUAD_VAR_MIN_VOICES")
# kind -> the switches it sets beside the minimums
KINDS = {"pwm": {}, "saw-pure": {}, "adapter": {}, "transform-per-voice": {}, "svf": {}, "svf-walk": {"SVF_WALK_MIN_ROWS": 4},
         "swept-walk": {"BIQUAD_VAR_WALK_MIN_ROWS": 4}, "sine-gate": {}, "stereo-biquad": {}, "stereo-ladder": {}}


def script(block):
    return [(i * block, block) for i in range(4)] + [(block, block)]


SCRIPTS = {"blocks": (script(1024), False), "windows": (script(4096), True)}
CASES = [f"{kind}:{pulls}" for kind in KINDS for pulls in SCRIPTS]


def voices(pg, kind):
    from pygmu2_amd.biquad_pe import BiquadMode
    from pygmu2_amd.transforms import Affine
    f = [110.0 * 2 ** (i / 12.0) for i in range(K)]
    r = [0.5 + 0.25 * i for i in range(K)]
    if kind == "pwm":
        return [pg.AnalogOscPE(f[i], duty_cycle=pg.TransformPE(pg.SinePE(r[i]), func=Affine(0.4, 0.5)), waveform="rectangle")
                for i in range(K)]
    if kind == "saw-pure":
        return [pg.AnalogOscPE(f[i], waveform="sawtooth") for i in range(K)]
    if kind == "adapter":
        return [pg.SpatialPE(pg.SinePE(f[i]), method=pg.SpatialAdapter(2)) for i in range(K)]
    if kind == "transform-per-voice":
        return [pg.TransformPE(pg.SinePE(r[i]), func=Affine(300.0, 100.0 * i)) for i in range(K)]
    if kind in ("svf", "svf-walk"):
        return [pg.SVFilterPE(pg.BlitSawPE(f[i]), 1000.0 + i, 2.0, BiquadMode.LOWPASS) for i in range(K)]
    if kind == "swept-walk":
        import test_noise_bank_trace
        return test_noise_bank_trace.voices(pg, "swept")
    if kind == "sine-gate":
        return [pg.GainPE(pg.SinePE(f[i]), gain=pg.AdsrGatedPE(pg.SinePE(2.0 + i), 0.01, 0.02, 0.5, 0.05)) for i in range(K)]
    if kind == "stereo-biquad":
        return [pg.BiquadPE(pg.SinePE(f[i], channels=2), 1000.0, 0.7) for i in range(K)]
    if kind == "stereo-ladder":
        return [pg.LadderPE(pg.SinePE(f[i], channels=2), 1000.0 + 50.0 * i, 0.3) for i in range(K)]
    raise KeyError(kind)


def run_case(monkeypatch, name):
    """-> the canonical trace of case `name`."""
    import pygmu2_amd as pg
    kind, pulls = name.split(":")
    pulls, mix_windows = SCRIPTS[pulls]
    return run(monkeypatch, lambda: voices(pg, kind), pulls, switches={**{minimum: 4 for minimum in MINIMUMS}, **KINDS[kind]},
               mix_windows=mix_windows)


def _calls(trace, name):
    return [entry for entry in trace if entry[0] == name]


def _buffers(trace):
    """The buffers a trace names: "b<k>" of every "b<k>+<offset>" argument."""
    return {arg.split("+")[0] for entry in trace for arg in entry[2:] if isinstance(arg, str) and "+" in arg}


def _pulls(trace):
    """The launches of each pull: [[entry, ...] per pull]."""
    at = [i for i, e in enumerate(trace) if e[0] == "pull"] + [len(trace)]
    return [[e for e in trace[a:b] if e[0].startswith("pgx_")] for a, b in zip(at, at[1:])]


@pytest.mark.parametrize("name", CASES)
def test_launch_trace(monkeypatch, name):
    assert_matches(name, run_case(monkeypatch, name), recorded(FIXTURE)[name])


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_a_stateful_analog_osc_bank_is_one_call_behind_its_modulators(monkeypatch, pulls):
    """[name, stream, out, out_stride, batch, start, n, channels, sr, wave, params, freq, freq_stride, duty, duty_stride,
    stateful, restart, state, workspace]"""
    trace = run_case(monkeypatch, f"pwm:{pulls}")
    for entries in _pulls(trace):
        names = [e[0] for e in entries if e[0] != "pgx_memcpy_d2d"]
        rendered = names.count("pgx_analog_osc_bank")              # (uniform ops: pgx_transform)
        assert names == ["pgx_sine_render", "pgx_transform", "pgx_analog_osc_bank", "pgx_mix_batch"] * rendered
    calls = _calls(trace, "pgx_analog_osc_bank")
    assert all(c[4] == K and c[9] == 0 and c[11] is None and c[13] is not None and c[15] == 1 for c in calls)
    assert all(c[17] is not None and c[18] is not None for c in calls)
    assert [c[16] for c in calls][:2] == [1, 0]                    # the first render restarts, the next continues
    if pulls == "windows":
        assert any(e[5] for e in _calls(trace, "return"))          # (it does get windows)


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_a_pure_sawtooth_bank_opens_no_window(monkeypatch, pulls):
    trace = run_case(monkeypatch, f"saw-pure:{pulls}")
    returns = _calls(trace, "return")                              # [name, stream, pointer, frames, channels, window row?]
    assert len(returns) == 5 and not any(e[5] for e in returns)
    block = SCRIPTS[pulls][0][0][1]
    calls = _calls(trace, "pgx_analog_osc_bank")
    assert [(c[5], c[6]) for c in calls] == SCRIPTS[pulls][0] and block == calls[0][6]       # exactly the requests
    assert all(c[15] == 0 and c[17] is None for c in calls)        # not stateful: no state


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_the_adapter_is_one_launch_over_the_stacked_frames(monkeypatch, pulls):
    """[name, stream, out, in, frames, in_channels, out_channels]"""
    trace = run_case(monkeypatch, f"adapter:{pulls}")
    calls = _calls(trace, "pgx_channel_adapt")
    assert calls and all((c[5], c[6]) == (1, 2) and c[4] % K == 0 for c in calls)
    assert all(e[4] == 2 for e in _calls(trace, "return"))


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_per_voice_ops_take_the_bank_entry(monkeypatch, pulls):
    trace = run_case(monkeypatch, f"transform-per-voice:{pulls}")
    assert _calls(trace, "pgx_transform_bank") and not _calls(trace, "pgx_transform")


@pytest.mark.parametrize("pulls", list(SCRIPTS))
@pytest.mark.parametrize("kind, entry", [("svf", "pgx_svf_bank"), ("svf-walk", "pgx_svf_bank"),
                                         ("swept-walk", "pgx_biquad_varying_bank")])
def test_the_walk_passes_no_workspace(monkeypatch, kind, entry, pulls):
    """The last argument of both entries is the workspace: the segmented plan's, or None -- every row walked."""
    if kind == "svf-walk":
        with pytest.MonkeyPatch.context() as other:                # (the threshold as it is, put back before it is lowered)
            segmented = run_case(other, f"svf:{pulls}")
    trace = run_case(monkeypatch, f"{kind}:{pulls}")
    calls = _calls(trace, entry)
    assert calls
    if kind == "svf":
        assert all(c[-1] is not None for c in calls)
        assert len({c[-1] for c in calls}) == 1                    # (one scratch buffer: the stand-in's 65536 bytes suffice)
    else:
        assert all(c[-1] is None for c in calls)
    if kind == "svf-walk":
        # ... and no scratch buffer is made: the segmented plan's trace names exactly one buffer more
        assert len(_buffers(segmented)) == len(_buffers(trace)) + 1


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_a_gate_that_is_no_periodic_gate_is_walked_beside_the_voices(monkeypatch, pulls):
    """The un-fused gate: fork, the gate's rows and pgx_adsr_gated on the side stream, the voices on the main stream, join,
    then the multiply fused into the mix."""
    trace = run_case(monkeypatch, f"sine-gate:{pulls}")
    assert not _calls(trace, "pgx_adsr_gated_periodic") and not _calls(trace, "pgx_adsr_gated_periodic_to")
    rendered = 0
    for entries in _pulls(trace):
        names = [(e[0], e[1]) for e in entries if e[0] != "pgx_memcpy_d2d"]
        while names:
            assert names[:7] == [("pgx_stream_fork", 0), ("pgx_sine_render", 1), ("pgx_adsr_gated", 1), ("pgx_stream_select", 1),
                                 ("pgx_sine_render", 0), ("pgx_stream_join", 0), ("pgx_gain_mix_batch", 0)], names[:7]
            names = names[7:]
            rendered += 1
    assert rendered >= 5


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_a_stereo_biquad_bank_takes_the_constant_kernel(monkeypatch, pulls):
    """[name, stream, out, out_stride, in, in_stride, batch, n, channels, coef, tables, settle, state, workspace]"""
    trace = run_case(monkeypatch, f"stereo-biquad:{pulls}")
    calls = _calls(trace, "pgx_biquad_const")
    assert calls and all((c[6], c[8]) == (K, 2) and c[3] == c[5] == 2 * c[7] for c in calls)
    assert not _calls(trace, "pgx_voice_tiles") and all(e[4] == 2 for e in _calls(trace, "return"))


def test_the_state_of_a_stereo_biquad_bank(monkeypatch):
    import pygmu2_amd as pg
    from pygmu2_amd import config, voice_bank
    install(monkeypatch, recording=False)
    monkeypatch.setattr(config, "_sample_rate", 48000)
    bank = voice_bank.try_build_bank(voices(pg, "stereo-biquad"))
    assert type(bank.root).__name__ == "_BiquadNode" and bank.root.state is None
    bank.render_mix(0, 1024)
    assert bank.root.state.shape == (K, 2, 2)


@pytest.mark.parametrize("pulls", list(SCRIPTS))
def test_a_stereo_ladder_bank(monkeypatch, pulls):
    """[name, stream, out, out_stride, in, in_stride, batch, n, channels, ...]"""
    trace = run_case(monkeypatch, f"stereo-ladder:{pulls}")
    calls = _calls(trace, "pgx_ladder")
    assert calls and all((c[6], c[8]) == (K, 2) and c[3] == c[5] == 2 * c[7] for c in calls)


def test_fixture_has_every_case_once():
    assert recorded_names(FIXTURE) == CASES


if __name__ == "__main__":
    record_main(FIXTURE, CASES, run_case)
