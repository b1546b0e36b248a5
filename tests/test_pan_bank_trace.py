"""
CPU: what a bank of panned voices launches -- pinned against a recorded trace, with the stand-ins of
tests/bank_trace.py (its Recorder, Library and buffers: no device).

Graphs (tests/pan_cases.py), five voices each:
    scalar   SpatialPE(SinePE, SpatialConstantPower(azimuth=a_i))                       a _PanNode root, gains
    lfo      SpatialPE(BiquadPE(BlitSawPE), SpatialLinear(azimuth=SinePE))              a _PanNode root, azimuth rows
    nested   GainPE(SpatialPE(SinePE, SpatialConstantPower(azimuth=a_i)), 0.5)          the pan as a level
Pull script: four contiguous pulls of 1 024 frames, then a seek back to frame 1 024.

Pinned beside the recorded launches: a block of a pan root is exactly ONE pgx_pan_mix_batch with batch 5 and no
pgx_mix_batch (no pgx_pan_bank either: there is no [K][n][2] layer); the nested graph is one pgx_pan_bank and one
pgx_mix_batch per block; pgx_pan_gains runs once, when the bank is built; nothing is uploaded after that.  The keying and
decline rules of voice_bank's SpatialPE kind are asserted on _signature / try_build_bank directly.

    python tests/test_pan_bank_trace.py --record        writes tests/golden/pan_bank_trace.json
"""

import os
import sys

import pytest

sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (oracle.golden_cases.S, run as a script)
import pan_cases                                          # noqa: E402
from bank_trace import assert_matches, install, record_main, recorded, recorded_names, run      # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pan_bank_trace.json")
K = pan_cases.K
BLOCK = 1024
PULLS = [(i * BLOCK, BLOCK) for i in range(4)] + [(BLOCK, BLOCK)]
CASES = ["scalar", "lfo", "nested"]


def build_voices(kind, count=K):
    import spec_build
    return [spec_build.build(pan_cases.voice(kind, i)) for i in range(count)]


def run_case(monkeypatch, kind):
    """-> the canonical trace of case `kind`."""
    assert pan_cases.SR == 48000                                  # (bank_trace.run's rate)

    def built(bank):
        assert type(bank.root).__name__ == pan_cases.ROOTS[kind]

    trace = run(monkeypatch, lambda: build_voices(kind), PULLS, built=built)
    returns = [e for e in trace if e[0] == "return"]              # [name, stream, pointer, frames, channels, window row?]
    assert len(returns) == len(PULLS) and all((e[3], e[4]) == (BLOCK, 2) for e in returns)
    return trace


def _blocks(trace):
    """The entries of each pull, 'free' left out: [[entry, ...] per pull]."""
    at = [i for i, e in enumerate(trace) if e[0] == "pull"] + [len(trace)]
    return [[e for e in trace[a:b] if e[0] not in ("free", "pull", "return")] for a, b in zip(at, at[1:])]


@pytest.mark.parametrize("name", CASES)
def test_launch_trace(monkeypatch, name):
    assert_matches(name, run_case(monkeypatch, name), recorded(FIXTURE)[name])


@pytest.mark.parametrize("kind", ["scalar", "lfo"])
def test_a_pan_root_block_is_one_fused_launch(monkeypatch, kind):
    """[name, stream, out, in, in_stride, batch, n, src_channels, gains, azimuth_stream, az_stride, constant_power]"""
    trace = run_case(monkeypatch, kind)
    blocks = _blocks(trace)
    assert len(blocks) == len(PULLS)
    for entries in blocks:
        names = [e[0] for e in entries]
        assert names.count("pgx_pan_mix_batch") == 1 and names[-1] == "pgx_pan_mix_batch"
        assert "pgx_mix_batch" not in names and "pgx_pan_bank" not in names and "pgx_pan" not in names
        call = entries[-1]
        assert call[1] == 0                                       # the main stream
        assert (call[4], call[5], call[6], call[7]) == (BLOCK, K, BLOCK, 1)
        if kind == "scalar":
            assert call[8] is not None and call[9] is None and call[11] == 1
            assert names == ["pgx_sine_render", "pgx_pan_mix_batch"]
        else:
            assert call[8] is None and call[9] is not None and (call[10], call[11]) == (BLOCK, 0)
            assert names.count("pgx_sine_render") == 1            # the five LFOs: one launch
    gains = {entries[-1][8] for entries in blocks}
    assert len(gains) == 1                                        # the buffer pgx_pan_gains wrote when the bank was built


def test_a_pan_level_is_one_pan_bank_and_one_mix(monkeypatch):
    """[pgx_pan_bank, stream, out, out_stride, in, in_stride, batch, n, src_channels, gains, azimuth_stream, az_stride,
    constant_power]"""
    trace = run_case(monkeypatch, "nested")
    for entries in _blocks(trace):
        names = [e[0] for e in entries]
        assert names == ["pgx_sine_render", "pgx_pan_bank", "pgx_gain_const", "pgx_mix_batch"]
        call = entries[1]
        assert (call[3], call[5], call[6], call[7], call[8]) == (2 * BLOCK, BLOCK, K, BLOCK, 1)
        assert call[9] is not None and call[10] is None and call[12] == 1
        mixed = entries[3]                                        # [name, stream, out, in, in_stride, batch, n_elems]
        assert (mixed[4], mixed[5], mixed[6]) == (2 * BLOCK, K, 2 * BLOCK)


@pytest.mark.parametrize("kind", CASES)
def test_gains_once_and_nothing_uploaded_per_block(monkeypatch, kind):
    """(A BlitSawPE bank uploads its initial states where a render does not continue the last one -- the first pull and
    the seek of `lfo` --: blit_saw_pe.py's reset rule, not a block's.)"""
    trace = run_case(monkeypatch, kind)
    at = [i for i, e in enumerate(trace) if e[0] == "pull"]
    built = trace[:at[0]]
    made = [e for e in trace if e[0] == "pgx_pan_gains"]
    if kind == "lfo":
        assert not made
    else:
        assert len(made) == 1 and made[0] in built
        assert made[0][4] == K and made[0][5] == 1                # [name, stream, gains, azimuth, batch, constant_power]
        uploads = [e for e in built if e[0] == "h2d"]
        assert made[0][3] in [e[2] for e in uploads]              # the azimuths: uploaded in front of it
    streamed = trace[at[1]:at[4]] if kind == "lfo" else trace[at[0]:]
    assert not [e for e in streamed if e[0] == "h2d"]


# ------------------------------------------------------------------------------------------ keying and declines
def _signature(monkeypatch, spec):
    import spec_build
    from pygmu2_amd import config, voice_bank
    monkeypatch.setattr(config, "_sample_rate", pan_cases.SR)
    return voice_bank._signature(spec_build.build(spec))


def test_keys(monkeypatch):
    from pan_cases import S, lfo, pan, sine
    sig = lambda spec: _signature(monkeypatch, spec)
    linear, power = sig(pan(sine(0), "linear", 10.0)), sig(pan(sine(0), "constant_power", 10.0))
    assert linear is not None and power is not None and linear != power          # the method class
    assert linear[0] == power[0] == "pan"
    assert sig(pan(sine(1), "linear", -70.0)) == linear                           # the azimuth itself is data
    swept = sig(pan(sine(0), "linear", lfo(0)))
    assert swept is not None and swept != linear                                  # ... whether it is a PE is not
    assert sig(pan(sine(0), "linear", dict(lfo(0), channels=2))) is None          # an (n, 1) stream only
    assert sig(pan(sine(0, 3), "linear", 10.0)) != linear                         # (the source's key is part of it)
    assert sig(S("SpatialPE", source=sine(0), method="hrtf", azimuth=30.0)) is None
    two, four = (sig(S("SpatialPE", source=sine(0), method="adapter", channels=c)) for c in (2, 4))
    assert two is not None and two[0] == "adapt" and two != four                  # the output channel count


def test_minimum_is_the_largest_of_the_tree(monkeypatch):
    import spec_build
    from pygmu2_amd import config, voice_bank
    monkeypatch.setattr(config, "_sample_rate", pan_cases.SR)
    assert voice_bank._min_voices(spec_build.build(pan_cases.voice("scalar", 0))) == voice_bank.MIN_VOICES
    noisy = pan_cases.pan(pan_cases.S("NoisePE", seed=1), "linear", 0.0)
    assert voice_bank._min_voices(spec_build.build(noisy)) == voice_bank.NOISE_MIN_VOICES


@pytest.mark.parametrize("kind", pan_cases.DECLINED)
def test_declined(monkeypatch, kind):
    import spec_build
    from pygmu2_amd import config, voice_bank
    install(monkeypatch, recording=False)
    monkeypatch.setattr(config, "_sample_rate", pan_cases.SR)
    mix = spec_build.build(pan_cases.declined(kind))
    assert voice_bank.try_build_bank(mix.inputs()) is None
    assert mix._voice_bank() is False


@pytest.mark.parametrize("kind", list(pan_cases.ROOTS))
def test_banked(monkeypatch, kind):
    import spec_build
    from pygmu2_amd import config, voice_bank
    install(monkeypatch, recording=False)
    monkeypatch.setattr(config, "_sample_rate", pan_cases.SR)
    mix = spec_build.build(pan_cases.mix(kind))
    bank = mix._voice_bank()
    assert bank and type(bank.root).__name__ == pan_cases.ROOTS[kind]
    assert voice_bank.try_build_bank(mix.inputs()[:3]) is None                    # below MIN_VOICES


def test_the_fused_root_can_be_switched_off(monkeypatch):
    """FUSED_PAN_MIX = False (what tools/pan_bank_probe.py compares with): the layer and the plain mix."""
    from pygmu2_amd import config, voice_bank
    rec = install(monkeypatch)
    monkeypatch.setattr(config, "_sample_rate", pan_cases.SR)
    monkeypatch.setattr(voice_bank, "FUSED_PAN_MIX", False)
    bank = voice_bank.try_build_bank(build_voices("scalar"))
    bank.render_mix(0, BLOCK)
    names = [e[0] for e in rec.entries if e[0].startswith("pgx_")]
    assert names == ["pgx_pan_gains", "pgx_sine_render", "pgx_pan_bank", "pgx_mix_batch"]


def test_the_abi_of_the_pan_entries():
    """The header entry is the binding (pygmu2_amd/_abi.py), and the built library exports the three."""
    import ctypes as C

    from pygmu2_amd import device
    ptr, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    rows = [ptr, i64, i32, i64, i32, ptr, ptr, i64, i32]          # in, in_stride, batch, n, src_channels, gains, az, az_stride, mode
    want = {"pgx_pan_gains": [ptr, ptr, i32, i32], "pgx_pan_bank": [ptr, i64] + rows, "pgx_pan_mix_batch": [ptr] + rows}
    library = device.load_library()
    for name, args in want.items():
        assert device._ABI.functions[name] == (C.c_int, args), name
        assert name in device.EXPORTED_SYMBOLS and hasattr(library, name), name


def test_spatial_pe_exposes_its_azimuth_read_only():
    import pygmu2_amd as pg
    lfo = pg.SinePE(1.0)
    assert pg.SpatialPE(pg.SinePE(), method=pg.SpatialLinear(azimuth=lfo))._azimuth is lfo
    assert pg.SpatialPE(pg.SinePE(), method=pg.SpatialConstantPower(azimuth=-30.0))._azimuth == -30.0
    adapted = pg.SpatialPE(pg.SinePE(), method=pg.SpatialAdapter(2))
    assert adapted._azimuth is None
    with pytest.raises(AttributeError):
        adapted._azimuth = 1.0


def test_the_probe_records_give_no_pan_minimum():
    """tools/pan_bank_probe.py's rule over its committed records (profiles/pan_bank_probe.jsonl): the bank is not slower
    than the per-voice path from MIN_VOICES voices on in any graph, which is why voice_bank has no PAN_MIN_VOICES."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import pan_bank_probe as probe
    finally:
        sys.path.pop(0)
    from pygmu2_amd import voice_bank
    records = probe.read_records(os.path.join(root, "profiles", "pan_bank_probe.jsonl"))
    assert {(r["kind"], r["voices"], r["block"]) for r in records} == \
        {(kind, k, block) for kind in probe.KINDS for k in probe.VOICES for block in probe.BLOCKS}
    for kind in probe.KINDS:
        assert probe.winning_minimum([r for r in records if r["kind"] == kind]) == voice_bank.MIN_VOICES, kind
    assert not hasattr(voice_bank, "PAN_MIN_VOICES")
    # the rule itself: slower only beyond the spread of the passes; a losing row ends the run of winning K
    row = lambda k, bank, off: {"voices": k, "bank_us_per_block": bank[1], "off_us_per_block": off[1],
                                "bank_runs_us": list(bank), "off_runs_us": list(off)}
    assert not probe.slower(row(4, (9, 10, 11), (8, 9.5, 10)))            # within the spread
    assert probe.slower(row(4, (11, 12, 13), (8, 9, 10)))
    rows = [row(4, (1, 1, 1), (2, 2, 2)), row(8, (3, 3, 3), (2, 2, 2)), row(16, (1, 1, 1), (2, 2, 2))]
    assert probe.winning_minimum(rows) == 16 and probe.winning_minimum(rows[:1]) == 4
    assert probe.winning_minimum(rows[:2]) is None


def test_fixture_has_every_case_once():
    assert recorded_names(FIXTURE) == CASES


if __name__ == "__main__":
    record_main(FIXTURE, CASES, run_case)
