"""Host: which modulated SinePE voices -- a PE-valued frequency, amplitude or phase: FM, AM, PM -- the voice bank takes
(voice_bank._signature, the "sine_mod" kind), what keeps two voices out of one launch, when the node forbids windows, and
the C ABI entries of the batched stateful sine."""

import pygmu2_amd as pg
from pygmu2_amd import device, voice_bank
from pygmu2_amd.transforms import Affine

sig = voice_bank._signature


def _mod(i=0, depth=200.0, centre=440.0, **kw):
    """The modulator of a two-operator FM voice: a sine scaled to `centre` +- `depth` Hz."""
    return pg.TransformPE(pg.SinePE(frequency=110.0 + 7.0 * i, **kw), func=Affine(depth, centre))


def _fm(i=0):
    return pg.SinePE(frequency=_mod(i, 150.0 + 10.0 * i, 300.0 + 50.0 * i), amplitude=0.2 + 0.01 * i)


def test_modulated_sines_have_a_signature():
    pg.set_sample_rate(48000)
    assert sig(_fm()) is not None
    assert sig(_fm())[0] == "sine_mod"
    assert sig(pg.SinePE(440.0, amplitude=_mod(0, 0.4, 0.5))) is not None
    assert sig(pg.SinePE(440.0, phase=_mod(0, 1.5, 0.0))) is not None
    assert sig(pg.SinePE(_mod(0), _mod(1, 0.4, 0.5), _mod(2, 1.5, 0.0), channels=2)) is not None
    # nested FM: a modulator that is itself a modulated sine has the same kind
    nested = pg.SinePE(frequency=pg.TransformPE(_fm(3), func=Affine(900.0, 660.0)))
    assert sig(nested) is not None and sig(nested)[0] == "sine_mod"
    # under whatever is above it
    envelope = pg.AdsrTriggeredPE(pg.PeriodicTrigger(2.0), 0.005, 0.3, 0.0, 0.1)
    assert sig(pg.GainPE(_fm(), gain=envelope)) is not None


def test_scalar_sines_keep_their_key():
    pg.set_sample_rate(48000)
    assert sig(pg.SinePE(440.0)) == ("sine", 1)
    assert sig(pg.SinePE(220.0, 0.3, 0.5, channels=2)) == ("sine", 2)


def test_keys_tell_which_parameters_are_pes_and_the_channel_count():
    pg.set_sample_rate(48000)
    freq, amp, phase = (pg.SinePE(_mod()), pg.SinePE(440.0, amplitude=_mod()), pg.SinePE(440.0, phase=_mod()))
    both = pg.SinePE(_mod(), amplitude=_mod())
    assert len({sig(freq), sig(amp), sig(phase), sig(both)}) == 4
    assert sig(freq) != sig(pg.SinePE(_mod(), channels=2))
    assert sig(freq)[1:5] == (1, True, False, False) and sig(phase)[1:5] == (1, False, False, True)


def test_keys_ignore_the_scalars():
    pg.set_sample_rate(48000)
    assert sig(_fm(0)) == sig(_fm(3))
    assert sig(pg.SinePE(_mod(0), 0.2, 0.0)) == sig(pg.SinePE(_mod(5, 90.0, 1000.0), 0.9, 1.25))
    assert sig(pg.SinePE(330.0, amplitude=_mod())) == sig(pg.SinePE(1200.5, amplitude=_mod(2)))


def test_what_is_not_batchable():
    pg.set_sample_rate(48000)
    assert sig(pg.SinePE(_mod(channels=2))) is None                                  # a two-channel modulator
    assert sig(pg.SinePE(440.0, amplitude=pg.SinePE(3.0, channels=2))) is None
    assert sig(pg.SinePE(pg.CropPE(_mod(), 0, 1000))) is None                        # a finite-extent modulator
    assert sig(pg.SinePE(pg.TransformPE(pg.SinePE(5.0), func=lambda v: 440.0 + v))) is None


def test_banks_are_built_or_declined_on_the_host_rules(monkeypatch):
    pg.set_sample_rate(48000)
    monkeypatch.setattr(voice_bank, "SINE_MOD_MIN_VOICES", 6)
    assert voice_bank._min_voices(_fm()) == 6
    assert voice_bank._min_voices(pg.GainPE(_fm(), 0.5)) == 6
    assert voice_bank._min_voices(pg.SinePE(440.0)) == voice_bank.MIN_VOICES
    assert voice_bank.try_build_bank([_fm(i) for i in range(5)]) is None             # below SINE_MOD_MIN_VOICES
    mixed = [_fm(i) if i != 2 else pg.SinePE(440.0, amplitude=_mod(i, 0.4, 0.5)) for i in range(6)]
    assert sig(mixed[2]) is not None
    assert voice_bank.try_build_bank(mixed) is None                                  # mixed shapes
    shared = _mod()
    assert voice_bank.try_build_bank([pg.SinePE(shared, 0.1 + 0.01 * i) for i in range(6)]) is None
    voices = [_fm(i) for i in range(6)]
    seen = set()
    assert all(sig(v) == sig(voices[0]) and voice_bank._collect_ids(v, seen) for v in voices)


def test_a_phase_in_play_forbids_windows(monkeypatch):
    """SinePE._look_ahead_condition's rule, per bank: a phase PE, or any voice's scalar phase that is not 0, makes the
    carried phase depend on where the blocks are cut.  (The stand-ins of tests/bank_trace.py: no device.)"""
    from bank_trace import install
    from pygmu2_amd import config
    install(monkeypatch, recording=False)
    monkeypatch.setattr(config, "_sample_rate", 48000)
    monkeypatch.setattr(voice_bank, "SINE_MOD_MIN_VOICES", voice_bank.MIN_VOICES)

    def bank(voice):
        built = voice_bank.try_build_bank([voice(i) for i in range(5)])
        assert built is not None
        node = built.root if type(built.root) is voice_bank._SineModNode else built.root.children["source"]
        assert type(node) is voice_bank._SineModNode
        assert node.state.shape == (5, 2) and node._STATE == ("state",)
        assert node._REQUEST_DEPENDENT == built.request_dependent
        return built

    assert not bank(_fm).request_dependent
    assert not bank(lambda i: pg.SinePE(440.0 + i, amplitude=_mod(i, 0.4, 0.5))).request_dependent
    assert bank(lambda i: pg.SinePE(440.0 + i, phase=_mod(i, 1.5, 0.0))).request_dependent
    assert bank(lambda i: pg.SinePE(_mod(i), 0.3, 0.25 if i == 3 else 0.0)).request_dependent      # one voice's scalar phase
    assert bank(lambda i: pg.SinePE(_mod(i), _mod(i, 0.4, 0.5), _mod(i, 1.5, 0.0))).request_dependent
    # as a level under something else the rule still reaches the bank
    assert bank(lambda i: pg.GainPE(pg.SinePE(440.0 + i, phase=_mod(i, 1.5, 0.0)), 0.5)).request_dependent
    assert not bank(lambda i: pg.GainPE(_fm(i), 0.5)).request_dependent


def test_the_default_minimum_is_at_least_the_general_one():
    assert voice_bank.SINE_MOD_MIN_VOICES >= voice_bank.MIN_VOICES
    assert voice_bank.SINE_MOD_WALK_MIN_ROWS >= 1


def test_abi_of_the_batched_entry():
    names = ("pgx_sine_stateful_bank", "pgx_sine_stateful_bank_workspace_bytes")
    lib = device.load_library()
    for name in names:
        assert name in device._ABI.functions, name
        assert name in {entry[0] for entry in device._SIGNATURES}, name
        assert name in device.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert device.SINE_STATEFUL_PARAMS is device._ABI.struct("pgx_sine_stateful_params")
    # voice v's slice: {phase, initialised}, then one total per tile of 2 048 frames
    for n, tiles in ((1, 1), (2047, 1), (2048, 1), (2049, 2), (4097, 3), (48000, 24)):
        for b in (1, 5):
            assert lib.pgx_sine_stateful_bank_workspace_bytes(n, b) == b * (tiles + 2) * 8
    # the scratch the node passes is the export's size, at every block length and bank size it can meet
    for n in (1, 7, 1024, 2047, 2048, 2049, 3077, 4096, 4097, 6149, 48000, 8 * 48000, (1 << 20) + 1):
        for b in (1, 4, 5, 16, 255, 511):
            assert voice_bank._SineModNode.scratch_bytes(n, b) == lib.pgx_sine_stateful_bank_workspace_bytes(n, b), (n, b)
    for n, b in ((0, 5), (-3, 5), (2048, 0), (2048, -1), (0, 0)):
        assert lib.pgx_sine_stateful_bank_workspace_bytes(n, b) == 0
