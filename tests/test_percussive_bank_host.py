"""Host: which SVFilterPE voices and AdsrTriggeredPE(PeriodicTrigger) envelopes the voice bank takes
(voice_bank._signature), what is key and what is per-voice data, the measured minimums, and when try_build_bank
declines.  No device work."""

import pygmu2_amd as pg
from pygmu2_amd import device, voice_bank
from pygmu2_amd.biquad_pe import BiquadMode
from pygmu2_amd.transforms import Affine


def _saw(i=0, channels=1):
    return pg.BlitSawPE(109.37 * 2 ** (i / 12), channels=channels)


def _svf(i=0, **kw):
    return pg.SVFilterPE(_saw(i), 1200.0 + 40.0 * i, 2.0 + 0.1 * i, **kw)


def _biquad(i=0):
    return pg.BiquadPE(_saw(i), frequency=1500.0, q=2.0)


def _triggered(i=0):
    return pg.AdsrTriggeredPE(pg.PeriodicTrigger(3.0 + 0.17 * i), 0.005, 0.04, 0.05, 0.6, 0.08)


def _gated(i=0):
    return pg.AdsrGatedPE(pg.PeriodicGate(3.0 + 0.17 * i, 0.5), 0.01, 0.05, 0.6, 0.03)


def _modulator():
    return pg.TransformPE(pg.SinePE(0.7), func=Affine(400.0, 1200.0))


def test_constant_svf_voices_have_a_signature():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.SVFilterPE(pg.BlitSawPE(110.0), 1200.0, 2.0)) == ("svf", ("blitsaw", 1))
    assert voice_bank._signature(pg.SVFilterPE(_saw(channels=2), 1200.0, 2.0)) == ("svf", ("blitsaw", 2))
    assert voice_bank._signature(_svf()) != voice_bank._signature(_biquad())


def test_mode_gain_and_scalars_are_not_part_of_the_key():
    pg.set_sample_rate(48000)
    want = voice_bank._signature(_svf())
    modes = [m for m in BiquadMode if m != BiquadMode.ALLPASS]
    assert len(modes) == 7
    for i, mode in enumerate(modes):
        assert voice_bank._signature(_svf(i, mode=mode, gain_db=3.0 * (i % 3) - 3.0)) == want
    assert voice_bank._signature(pg.SVFilterPE(_saw(), 80.0, 0.5)) == want


def test_an_svf_with_a_pe_parameter_stays_per_voice():
    """(tests/test_swept_bank_host.py pins the frequency form; the node uploads host constants and runs no modulator)"""
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.SVFilterPE(_saw(), frequency=_modulator(), q=2.0)) is None
    assert voice_bank._signature(pg.SVFilterPE(_saw(), frequency=1200.0, q=pg.SinePE(2.0))) is None
    assert voice_bank._signature(pg.SVFilterPE(_saw(), frequency=_modulator(), q=pg.SinePE(2.0))) is None


def test_the_key_of_a_triggered_envelope():
    pg.set_sample_rate(48000)
    envelope = ("adsr_trig", ("trigger",))
    assert voice_bank._signature(pg.PeriodicTrigger(3.0, phase=0.25, amplitude=2)) == ("trigger",)
    assert voice_bank._signature(_triggered()) == envelope
    assert voice_bank._signature(_triggered(5)) == envelope                      # (rate and times are per-voice data)
    assert voice_bank._signature(pg.GainPE(_svf(), gain=_triggered())) == ("gain_pe", ("svf", ("blitsaw", 1)), envelope)
    cutoff = pg.TransformPE(_triggered(), func=Affine(2500.0, 300.0))
    sig = voice_bank._signature(cutoff)
    assert sig[0] == "transform" and sig[-1] == envelope
    swept = pg.GainPE(pg.BiquadPE(_saw(), frequency=cutoff, q=2.0), gain=_triggered(1))
    assert voice_bank._signature(swept) == ("gain_pe", ("biquad_var", True, False, ("blitsaw", 1), sig), envelope)
    assert voice_bank._signature(_gated()) != envelope


def test_the_minimums_are_the_measured_ones_and_switches(monkeypatch):
    pg.set_sample_rate(48000)
    for name in ("SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES"):
        assert getattr(voice_bank, name) >= voice_bank.MIN_VOICES
    assert voice_bank.SVF_WALK_MIN_ROWS >= 1
    assert voice_bank._min_voices(_svf()) == voice_bank.SVF_MIN_VOICES
    assert voice_bank._min_voices(pg.GainPE(_svf(), 0.5)) == voice_bank.SVF_MIN_VOICES
    assert voice_bank._min_voices(_triggered()) == voice_bank.ADSR_TRIGGERED_MIN_VOICES
    assert voice_bank._min_voices(pg.GainPE(_biquad(), gain=_triggered())) == voice_bank.ADSR_TRIGGERED_MIN_VOICES
    assert (voice_bank._min_voices(pg.GainPE(_svf(), gain=_triggered()))
            == max(voice_bank.SVF_MIN_VOICES, voice_bank.ADSR_TRIGGERED_MIN_VOICES))
    assert voice_bank._min_voices(_biquad()) == voice_bank.MIN_VOICES
    assert voice_bank._min_voices(pg.GainPE(_biquad(), gain=_gated())) == voice_bank.MIN_VOICES
    monkeypatch.setattr(voice_bank, "SVF_MIN_VOICES", 7)
    monkeypatch.setattr(voice_bank, "ADSR_TRIGGERED_MIN_VOICES", 9)
    assert voice_bank._min_voices(_svf()) == 7
    assert voice_bank._min_voices(_triggered()) == 9
    assert voice_bank._min_voices(pg.GainPE(_svf(), gain=_triggered())) == 9
    assert voice_bank.try_build_bank([_svf(i) for i in range(6)]) is None
    assert voice_bank.try_build_bank([pg.GainPE(_biquad(i), gain=_triggered(i)) for i in range(8)]) is None
    assert voice_bank.try_build_bank([_svf(i) for i in range(voice_bank.MIN_VOICES - 1)]) is None


def test_a_mixed_list_is_declined(monkeypatch):
    pg.set_sample_rate(48000)
    monkeypatch.setattr(voice_bank, "SVF_MIN_VOICES", voice_bank.MIN_VOICES)
    monkeypatch.setattr(voice_bank, "ADSR_TRIGGERED_MIN_VOICES", voice_bank.MIN_VOICES)
    under = lambda i, envelope: pg.GainPE(_biquad(i), gain=envelope(i))
    assert voice_bank.try_build_bank([under(i, _gated if i == 2 else _triggered) for i in range(5)]) is None
    assert voice_bank.try_build_bank([_svf(i) if i == 2 else _biquad(i) for i in range(5)]) is None
    assert voice_bank.try_build_bank([_biquad(i) if i == 2 else _svf(i) for i in range(5)]) is None
    shared = _triggered()
    assert voice_bank.try_build_bank([pg.GainPE(_svf(i), gain=shared) for i in range(5)]) is None    # a shared envelope


def test_the_nodes_are_plain():
    assert voice_bank._SvfNode._STATE == ("state",)
    assert voice_bank._AdsrTriggeredNode._STATE == ("state",)
    assert not issubclass(voice_bank._AdsrTriggeredNode, voice_bank._AdsrGatedNode)
    assert not issubclass(voice_bank._SvfNode, (voice_bank._BiquadNode, voice_bank._BiquadVarNode))
    for name in ("render_ahead", "take_ahead", "mark_consumed", "fused_gate", "forget_ahead"):
        assert not hasattr(voice_bank._AdsrTriggeredNode, name)


def test_the_on_chip_mix_rule_takes_a_triggered_gain():
    """GainPE(BiquadPE(BlitSawPE), gain=<any mono PE>): the rule looks at the chain, not at the envelope's class."""
    pg.set_sample_rate(48000)
    triggered = [pg.GainPE(_biquad(i), gain=_triggered(i)) for i in range(16)]
    gated = [pg.GainPE(_biquad(i), gain=_gated(i)) for i in range(16)]
    assert voice_bank.on_chip_mix_rule(triggered) == voice_bank.on_chip_mix_rule(gated)
    assert not voice_bank.on_chip_mix_rule([pg.GainPE(_svf(i), gain=_triggered(i)) for i in range(16)])


def test_abi_of_the_two_entries():
    for name in ("pgx_svf_bank", "pgx_periodic_trigger_bank"):
        assert name in device._ABI.functions
        assert name in device.EXPORTED_SYMBOLS
        assert hasattr(device.load_library(), name)
    assert len(device._ABI.functions["pgx_svf_bank"][1]) == 17
    assert len(device._ABI.functions["pgx_periodic_trigger_bank"][1]) == 8
