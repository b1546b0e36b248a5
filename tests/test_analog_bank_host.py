"""Host: which AnalogOscPE / TransformPE voice trees the voice bank takes (voice_bank._signature), what keeps two voices
out of one launch, and the C ABI entries of the batched oscillator and transform."""

import pygmu2_amd as pg
from pygmu2_amd import device, voice_bank
from pygmu2_amd.transforms import Affine, Chain, PitchToFreq, Tanh


def _lfo(i=0, **kw):
    return pg.TransformPE(pg.SinePE(frequency=0.7 + 0.31 * i, **kw), func=Affine(0.4, 0.5))


def test_analog_osc_voices_have_a_signature():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.AnalogOscPE(109.37, 0.2)) is not None
    assert voice_bank._signature(pg.AnalogOscPE(109.37, 0.2, "sawtooth", channels=2)) is not None
    assert voice_bank._signature(pg.AnalogOscPE(109.37, duty_cycle=_lfo())) is not None
    assert voice_bank._signature(_lfo()) is not None
    envelope = pg.AdsrGatedPE(pg.PeriodicGate(3.0, 0.5), 0.01, 0.05, 0.6, 0.03)
    pitch = pg.TransformPE(envelope, func=Affine(300.0, 109.37))
    assert voice_bank._signature(pg.AnalogOscPE(pitch, 0.3)) is not None


def test_what_is_not_batchable():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.TransformPE(pg.SinePE(1.0), func=lambda v: 0.5 + 0.4 * v)) is None
    assert voice_bank._signature(pg.TransformPE(pg.SinePE(1.0), func=Chain(Affine(12.0, 60.0), PitchToFreq()))) is None
    explicit = PitchToFreq(pg.temperament.EqualTemperament(12), 69.0, 440.0)      # a tuning step: pgx_tuning's program
    assert voice_bank._signature(pg.TransformPE(pg.SinePE(1.0), func=Chain(Affine(12.0, 60.0), explicit))) is None
    assert voice_bank._signature(pg.TransformPE(pg.CropPE(pg.SinePE(1.0), 0, 100), func=Affine(0.4, 0.5))) is None
    assert voice_bank._signature(pg.AnalogOscPE(109.37, duty_cycle=_lfo(channels=2))) is None
    assert voice_bank._signature(pg.AnalogOscPE(pg.SinePE(3.0, channels=2), 0.5)) is None
    assert voice_bank._signature(pg.AnalogOscPE(109.37, duty_cycle=pg.TransformPE(pg.SinePE(1.0), func=lambda v: v))) is None


def test_keys_keep_unlike_voices_apart():
    pg.set_sample_rate(48000)
    sig = voice_bank._signature
    assert sig(pg.AnalogOscPE(109.37, 0.2)) == sig(pg.AnalogOscPE(220.1, 0.4))
    assert sig(pg.AnalogOscPE(109.37, 0.2)) != sig(pg.AnalogOscPE(109.37, 0.2, "sawtooth"))
    assert sig(pg.AnalogOscPE(109.37, 0.2)) != sig(pg.AnalogOscPE(109.37, 0.2, channels=2))
    assert sig(pg.AnalogOscPE(109.37, 0.2)) != sig(pg.AnalogOscPE(109.37, duty_cycle=_lfo()))
    # the same modulator on the other parameter is another voice shape
    assert sig(pg.AnalogOscPE(_lfo(), 0.2)) != sig(pg.AnalogOscPE(109.37, duty_cycle=_lfo()))
    a = pg.TransformPE(pg.SinePE(1.0), func=Affine(0.4, 0.5))
    b = pg.TransformPE(pg.SinePE(1.0), func=Tanh())
    c = pg.TransformPE(pg.SinePE(1.0), func=Chain(Affine(0.4, 0.5), Tanh()))
    assert len({sig(a), sig(b), sig(c)}) == 3
    # the steps are the key, their parameters are per voice (a pitch envelope's offset is the voice's frequency)
    assert sig(a) == sig(pg.TransformPE(pg.SinePE(2.0), func=Affine(300.0, 109.37)))


def test_banks_are_built_or_declined_on_the_host_rules():
    pg.set_sample_rate(48000)
    voices = [pg.AnalogOscPE(109.37 * 2 ** (i / 12), duty_cycle=_lfo(i)) for i in range(4)]
    assert all(voice_bank._signature(v) == voice_bank._signature(voices[0]) for v in voices)
    seen = set()
    assert all(voice_bank._collect_ids(v, seen) for v in voices)
    shared = _lfo()
    seen = set()
    assert not all(voice_bank._collect_ids(pg.AnalogOscPE(100.0 + i, duty_cycle=shared), seen) for i in range(4))
    assert voice_bank.try_build_bank([pg.AnalogOscPE(100.0 + i, 0.3) for i in range(voice_bank.MIN_VOICES - 1)]) is None
    mixed = [pg.AnalogOscPE(100.0 + i, 0.3, "sawtooth" if i == 2 else "rectangle") for i in range(5)]
    assert voice_bank.try_build_bank(mixed) is None


def test_the_minimum_of_a_tree_is_its_largest(monkeypatch):
    pg.set_sample_rate(48000)
    assert voice_bank.ANALOG_OSC_MIN_VOICES >= voice_bank.MIN_VOICES
    osc = pg.AnalogOscPE(109.37, duty_cycle=_lfo())
    assert voice_bank._min_voices(_lfo()) == voice_bank.MIN_VOICES
    assert voice_bank._min_voices(osc) == voice_bank.ANALOG_OSC_MIN_VOICES
    assert voice_bank._min_voices(pg.GainPE(pg.BiquadPE(osc, 1500.0, 0.9), 0.5)) == voice_bank.ANALOG_OSC_MIN_VOICES
    assert voice_bank._min_voices(pg.BiquadPE(pg.BlitSawPE(110.0), 1500.0, 0.9)) == voice_bank.MIN_VOICES
    voices = [pg.AnalogOscPE(100.0 + i, 0.3) for i in range(voice_bank.ANALOG_OSC_MIN_VOICES - 1)]
    assert voice_bank.try_build_bank(voices) is None
    monkeypatch.setattr(voice_bank, "ANALOG_OSC_MIN_VOICES", 7)
    assert voice_bank._min_voices(osc) == 7


def test_abi_of_the_batched_entries():
    names = ("pgx_analog_osc_bank", "pgx_analog_osc_bank_workspace_bytes", "pgx_transform_bank")
    lib = device.load_library()
    for name in names:
        assert name in device._ABI.functions, name
        assert name in device.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert device.OSC_PARAMS is device._ABI.struct("pgx_osc_params")
    assert device.OSC_PARAMS.itemsize == 16 and device.OSC_PARAMS.names == ("freq", "duty")
    for n in (1, 2047, 2048, 2049, 4101):
        for b in (1, 5):
            assert lib.pgx_analog_osc_bank_workspace_bytes(n, b) == b * lib.pgx_analog_osc_workspace_bytes(n)
    assert lib.pgx_analog_osc_workspace_bytes(2049) == 2 * (2 * 2 + 4) * 8          # (unchanged by the voice dimension)
    for n, b in ((0, 5), (-3, 5), (2048, 0), (2048, -1), (0, 0)):
        assert lib.pgx_analog_osc_bank_workspace_bytes(n, b) == 0
