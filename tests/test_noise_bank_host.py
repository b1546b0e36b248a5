"""Host: which NoisePE and FunctionGenPE voices the voice bank takes (voice_bank._signature), what is key and what is
per-voice data, the minimum of a tree that holds a NoisePE, when try_build_bank declines, and the ABI of
pgx_function_gen_bank.  No device work."""

import pygmu2_amd as pg
from pygmu2_amd import device, voice_bank
from pygmu2_amd.biquad_pe import BiquadMode
from pygmu2_amd.transforms import Affine

MODES = (pg.NoiseMode.WHITE, pg.NoiseMode.PINK, pg.NoiseMode.BROWN)


def _hihat(i=0):
    envelope = pg.AdsrTriggeredPE(pg.PeriodicTrigger(4.0 + 0.01 * i), 0.001, 0.02, 0.03, 0.3, 0.05)
    return pg.GainPE(pg.SVFilterPE(pg.NoisePE(seed=i), 6000.0 + 100.0 * i, 2.0, BiquadMode.HIGHPASS), gain=envelope)


def _lfo(channels=1):
    return pg.FunctionGenPE(0.5, 0.5, waveform="sawtooth", channels=channels)


def _holds(key, sub):
    return key == sub or (isinstance(key, tuple) and any(_holds(part, sub) for part in key))


# ---------------------------------------------------------------------------------------------- signatures
def test_noise_signatures_one_key_per_mode():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.NoisePE(seed=1)) == ("noise", "white")
    assert voice_bank._signature(pg.NoisePE(seed=1, mode=pg.NoiseMode.PINK)) == ("noise", "pink")
    assert voice_bank._signature(pg.NoisePE(seed=1, mode=pg.NoiseMode.BROWN)) == ("noise", "brown")
    assert len({voice_bank._signature(pg.NoisePE(seed=1, mode=m)) for m in MODES}) == 3


def test_range_and_seed_are_not_part_of_the_key():
    pg.set_sample_rate(48000)
    for mode in MODES:
        want = voice_bank._signature(pg.NoisePE(seed=1, mode=mode))
        assert want is not None
        assert voice_bank._signature(pg.NoisePE(-0.25, 3.0, seed=77, mode=mode)) == want
        assert voice_bank._signature(pg.NoisePE(seed=None, mode=mode)) == want
        assert voice_bank._signature(pg.NoisePE(0.0, 1.0, seed=2 ** 40, mode=mode)) == want


def test_function_gen_signatures():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(pg.FunctionGenPE(2.0, 0.3, waveform="sawtooth")) == ("function_gen", "sawtooth", 1)
    assert voice_bank._signature(pg.FunctionGenPE(2.0, 0.3, channels=3)) == ("function_gen", "rectangle", 3)
    assert voice_bank._signature(pg.FunctionGenPE(7.0, 0.9, phase=0.25, waveform="sawtooth")) == \
        voice_bank._signature(pg.FunctionGenPE(2.0, 0.3, waveform="sawtooth"))          # frequency, duty, phase: data
    # a PE parameter: the generator carries a phase and restarts on a seek -- PeriodicGate's rule
    assert voice_bank._signature(pg.FunctionGenPE(pg.SinePE(1.0))) is None
    assert voice_bank._signature(pg.FunctionGenPE(2.0, duty_cycle=pg.SinePE(1.0))) is None
    assert voice_bank._signature(pg.FunctionGenPE(2.0, phase=pg.SinePE(1.0))) is None


def test_function_gen_as_a_modulator_follows_the_one_channel_rule():
    pg.set_sample_rate(48000)

    def duty(source):
        return pg.AnalogOscPE(220.0, duty_cycle=pg.TransformPE(source, func=Affine(0.3, 0.5)))

    def cutoff(source):
        return pg.BiquadPE(pg.BlitSawPE(110.0), frequency=pg.TransformPE(source, func=Affine(2000.0, 2500.0)), q=2.0)

    for tree in (duty, cutoff):
        assert voice_bank._signature(tree(_lfo(channels=2))) is None
        key = voice_bank._signature(tree(_lfo()))
        assert key is not None and _holds(key, ("function_gen", "sawtooth", 1))
        assert key != voice_bank._signature(tree(pg.SinePE(0.5)))
    assert voice_bank._signature(pg.AnalogOscPE(220.0, duty_cycle=_lfo(channels=2))) is None
    assert voice_bank._signature(pg.AnalogOscPE(220.0, duty_cycle=_lfo())) is not None
    assert voice_bank._signature(pg.BiquadPE(pg.BlitSawPE(110.0), frequency=_lfo(channels=2), q=2.0)) is None
    # no minimum of its own: the parent's
    assert voice_bank._min_voices(_lfo()) == voice_bank.MIN_VOICES
    assert voice_bank._min_voices(duty(_lfo())) == voice_bank.ANALOG_OSC_MIN_VOICES
    assert voice_bank._min_voices(cutoff(_lfo())) == voice_bank.BIQUAD_VAR_MIN_VOICES


def test_the_hihat_voice():
    pg.set_sample_rate(48000)
    assert voice_bank._signature(_hihat()) == ("gain_pe", ("svf", ("noise", "white")), ("adsr_trig", ("trigger",)))
    assert voice_bank._signature(_hihat(3)) == voice_bank._signature(_hihat())
    assert voice_bank._min_voices(_hihat()) == max(voice_bank.NOISE_MIN_VOICES, voice_bank.SVF_MIN_VOICES,
                                                   voice_bank.ADSR_TRIGGERED_MIN_VOICES)
    assert voice_bank._min_voices(pg.NoisePE(seed=1)) == voice_bank.NOISE_MIN_VOICES >= voice_bank.MIN_VOICES


# ---------------------------------------------------------------------------------------------- try_build_bank declines
def test_try_build_bank_declines(monkeypatch):
    """(before anything of a bank is built: no device is touched)"""
    pg.set_sample_rate(48000)
    monkeypatch.setattr(voice_bank, "NOISE_MIN_VOICES", 6)
    assert voice_bank.try_build_bank([pg.NoisePE(seed=i, mode=pg.NoiseMode.PINK) for i in range(5)]) is None
    mixed = [pg.NoisePE(seed=i, mode=pg.NoiseMode.PINK) for i in range(7)] + [pg.NoisePE(seed=9, mode=pg.NoiseMode.BROWN)]
    assert voice_bank.try_build_bank(mixed) is None
    shared = pg.NoisePE(seed=3)
    voices = [pg.GainPE(shared, gain=0.5) for _ in range(8)]
    assert voice_bank._signature(voices[0]) is not None
    assert voice_bank.try_build_bank(voices) is None
    bounded = [pg.CropPE(pg.NoisePE(seed=i), 0, 1000) for i in range(8)]
    assert voice_bank.try_build_bank(bounded) is None


def test_a_mix_below_the_minimum_stays_per_voice():
    pg.set_sample_rate(48000)
    assert voice_bank.NOISE_MIN_VOICES >= voice_bank.MIN_VOICES == 4
    mix = pg.MixPE(*[pg.NoisePE(seed=i) for i in range(voice_bank.NOISE_MIN_VOICES - 1)])
    assert mix._voice_bank() is False


# ---------------------------------------------------------------------------------------------- what a node is told
def test_a_noise_pe_outside_a_bank_tells_nobody():
    pg.set_sample_rate(48000)
    pe = pg.NoisePE(seed=5)
    assert pe._bank_slot is None and pe._bank_node() is None
    pe.advance(10)
    pe.reset_state()
    assert pe._consumed == 0


def test_the_seed_record_is_what_the_pe_uploads():
    pg.set_sample_rate(48000)
    rec = pg.NoisePE(-0.5, 2.0, seed=11)._seed_record()
    assert rec.dtype == device.NOISE_PARAMS and rec.shape == (1,)
    assert int(rec["scaled"][0]) == 1 and float(rec["span"][0]) == 2.5 and float(rec["min_value"][0]) == -0.5
    assert int(rec["consumed"][0]) == 0
    assert int(pg.NoisePE(seed=11)._seed_record()["scaled"][0]) == 0
    a, b = pg.NoisePE(seed=None)._seed_record(), pg.NoisePE(seed=None)._seed_record()
    assert (int(a["state_hi"][0]), int(a["state_lo"][0])) != (int(b["state_hi"][0]), int(b["state_lo"][0]))


# ---------------------------------------------------------------------------------------------- ABI
def test_the_abi_of_the_function_gen_bank():
    assert "pgx_function_gen_bank" in device._ABI.functions
    assert "pgx_function_gen_bank" in device.EXPORTED_SYMBOLS
    assert hasattr(device.load_library(), "pgx_function_gen_bank")
    assert device.FUNCTION_GEN_PARAMS.itemsize == 24
    assert device.FUNCTION_GEN_PARAMS.names == ("dt", "phase", "duty")
    assert device.FUNCTION_GEN_PARAMS == device._ABI.struct("pgx_function_gen_params")
    import ctypes
    res, args = device._ABI.functions["pgx_function_gen_bank"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                    ctypes.c_int, ctypes.c_void_p]


def test_the_reader_takes_a_second_name_for_an_earlier_struct():
    """`typedef pgx_a pgx_b;`: pgx_function_gen_params is pgx_gate_params' record -- the same dtype, no table entry."""
    import pytest

    from pygmu2_amd import _abi

    def header(body):
        return '#ifdef __cplusplus\nextern "C" {\n#endif\n' + body + '\n#ifdef __cplusplus\n}\n#endif\n'

    abi = _abi.parse(header("typedef struct { double a; int32_t n; int32_t pad; } pgx_a;\ntypedef pgx_a pgx_b;\n"
                            "int pgx_f(const pgx_b *p, pgx_a *q);"))
    assert list(abi.structs) == ["pgx_a"] and abi.aliases == {"pgx_b": "pgx_a"}
    assert abi.struct("pgx_b") is abi.struct("pgx_a") and abi.struct("pgx_b").itemsize == 16
    import ctypes
    assert abi.functions["pgx_f"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    for body in ("typedef pgx_later pgx_b;", "typedef struct { double a; } pgx_a;\ntypedef pgx_a pgx_a;",
                 "typedef struct { double a; } pgx_a;\ntypedef pgx_a pgx_b;\ntypedef pgx_a pgx_b;"):
        with pytest.raises(_abi.AbiError, match="new name for an earlier struct"):
            _abi.parse(header(body))
    assert device._ABI.aliases == {"pgx_function_gen_params": "pgx_gate_params"}
    assert "pgx_function_gen_params" not in device._ABI.structs
