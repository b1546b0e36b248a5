"""GPU: a MixPE of AnalogOscPE voices -- pure, or with duty cycle / frequency driven by TransformPE modulators -- is
rendered as a voice bank (pgx_analog_osc_bank, pgx_transform / pgx_transform_bank) and gives the samples of the
per-voice path bit for bit: the same kernels with the voice in the grid, the same tiles, the same mix order.  The pure
sawtooth, whose samples depend on how the stream is cut into requests, is never windowed; the filter and gain levels
above take the new source through their general branch; the oracle bounds both paths.

Block lengths around the scan tile of 2048 frames (one tile, a full tile, one frame into the next, three tiles), a
seek before the last block; 4 (voice_bank.MIN_VOICES), 5 and once 70 voices; frequencies 109.37 * 2^(i/12), whose
periods are no whole number of frames (the restated phases stay >= 1e-6 from a waveform edge over these blocks).

By default a tree that holds an AnalogOscPE is banked from voice_bank.ANALOG_OSC_MIN_VOICES = 64 voices on (measured:
tools/analog_bank_probe.py).  The 70-voice case runs under that default; the small banks, where a wrong tile, voice
offset or state slot shows just as well, set the switch to MIN_VOICES (`small_banks`), as the tests of the other banks
set theirs."""

import numpy as np
import pytest

import pygmu2_amd as pg
from fuzz_graphs_all import osc_edge_distance
from oracle.golden_cases import S
from oracle.graph_eval import Node
from pygmu2_amd import look_ahead, voice_bank
from spec_build import build

pytestmark = pytest.mark.gpu

SR = 48000
BLOCKS = [(0, 4101), (4101, 2048), (6149, 1), (6150, 2047), (20000, 4101)]
FORMS = ("pure", "duty", "freq", "both")


@pytest.fixture
def small_banks(monkeypatch):
    monkeypatch.setattr(voice_bank, "ANALOG_OSC_MIN_VOICES", voice_bank.MIN_VOICES)


def _freq(i):
    return 109.37 * 2 ** (i / 12)


def _lfo(i):
    return S("TransformPE", source=S("SinePE", frequency=0.7 + 0.31 * i), ops=[["affine", 0.4, 0.5]])


def _envelope(i):
    return S("AdsrGatedPE", gate=S("PeriodicGate", frequency=3.0 + 0.17 * i, duty_cycle=0.5),
             attack_time=0.01, decay_time=0.05, sustain_level=0.6, release_time=0.03)


def _pitch(i):
    return S("TransformPE", source=_envelope(i), ops=[["affine", 300.0, _freq(i)]])


def _osc(i, form, wave, channels=1):
    return S("AnalogOscPE", frequency=_pitch(i) if form in ("freq", "both") else _freq(i),
             duty_cycle=_lfo(i) if form in ("duty", "both") else 0.2 + 0.1 * i,
             waveform=wave, channels=channels)


def _mix_spec(count, form, wave, channels=1, above=lambda i, osc: osc):
    return S("MixPE", inputs=[above(i, _osc(i, form, wave, channels)) for i in range(count)])


def _render_blocks(root, blocks=BLOCKS):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(root)
    r.start()
    out = [root.render(s, n).data.copy() for s, n in blocks]
    r.stop()
    return out


def _both_paths(spec, blocks=BLOCKS):
    """(the banked MixPE, its blocks, the blocks of a twin rendered voice by voice, the twin)"""
    pg.set_sample_rate(SR)
    banked = build(spec)
    got = _render_blocks(banked, blocks)
    assert banked._bank, "no voice bank was built"
    plain = build(spec)
    plain._bank = False
    return banked, got, _render_blocks(plain, blocks), plain


def _assert_equal(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        assert np.array_equal(a, b), f"{what} block {k}: max|d| = {np.max(np.abs(a.astype(np.float64) - b))}"


def _osc_node(bank):
    node = bank.root
    while not isinstance(node, voice_bank._AnalogOscNode):
        node = node.children["source"]
    return node


# ---------------------------------------------------------------------------------------- 1. the per-voice path, bit for bit
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
@pytest.mark.parametrize("form", FORMS)
def test_bank_equals_the_per_voice_path(form, wave, channels):
    for count in (4, 5):
        banked, got, want, _ = _both_paths(_mix_spec(count, form, wave, channels))
        root = banked._bank.root
        assert isinstance(root, voice_bank._AnalogOscNode) and root.k == count and root.stateful == (form != "pure")
        assert got[0].shape == (BLOCKS[0][1], channels)
        _assert_equal(got, want, f"{form} {wave} x{count}")


def test_seventy_stateful_sawtooth_voices():
    """(under the default minimum: 70 >= ANALOG_OSC_MIN_VOICES)"""
    assert voice_bank.MIN_VOICES <= voice_bank.ANALOG_OSC_MIN_VOICES <= 70
    banked, got, want, _ = _both_paths(_mix_spec(70, "both", "sawtooth"))
    assert banked._bank.root.k == 70
    _assert_equal(got, want, "70 voices")


@pytest.mark.usefixtures("small_banks")
def test_per_voice_transform_parameters_are_one_launch_each_level():
    """The duty modulators share one program (pgx_transform over the stacked voices); the pitch envelopes' offsets are
    per voice (pgx_transform_bank)."""
    banked, _, _, _ = _both_paths(_mix_spec(5, "both", "rectangle"), BLOCKS[:1])
    children = banked._bank.root.children
    assert isinstance(children["duty"], voice_bank._TransformNode) and children["duty"].uniform
    assert isinstance(children["frequency"], voice_bank._TransformNode) and not children["frequency"].uniform


# ---------------------------------------------------------------------------------------- 2. lifecycle
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
def test_stop_start_and_reset_state_give_the_same_samples_again(wave):
    def run(mix):
        first = _render_blocks(mix)
        again = _render_blocks(mix)                       # stop / start in between
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(mix)
        r.start()
        head = [mix.render(s, n).data.copy() for s, n in BLOCKS[:2]]
        mix.reset_state()
        after = [mix.render(s, n).data.copy() for s, n in BLOCKS]
        r.stop()
        return first, again, head, after

    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "duty", wave)
    banked, plain = build(spec), build(spec)
    plain._bank = False
    first, again, head, after = run(banked)
    assert banked._bank
    _assert_equal(again, first, "stop/start")
    _assert_equal(head, first[:2], "restart")
    _assert_equal(after, first, "reset_state")
    for got, want in zip((first, again, head, after), run(plain)):
        _assert_equal(got, want, "per-voice path")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
def test_a_seek_restarts_phase_and_saw_value_like_the_per_voice_path(wave):
    """The last block follows a seek: both paths restart at phase 0 / saw -1 there, and leave the same carried numbers."""
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "both", wave)
    last, states = [], []
    for bank_on in (True, False):
        mix = build(spec)
        if not bank_on:
            mix._bank = False
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(mix)
        r.start()
        for s, n in BLOCKS:
            block = mix.render(s, n).data.copy()
        last.append(block)
        if bank_on:
            node = _osc_node(mix._bank)
            assert node.last_end == BLOCKS[-1][0] + BLOCKS[-1][1]
            states.append(node.state.to_host())
        else:
            for voice in mix.inputs():
                look_ahead.before_direct_access(voice)
            states.append(np.stack([voice._state.to_host() for voice in mix.inputs()]))
        r.stop()
    assert np.array_equal(last[0], last[1])
    assert states[0].shape == states[1].shape == (5, 2) and np.array_equal(states[0], states[1])


# ---------------------------------------------------------------------------------------- 3. windows
STREAM = [(s, 4096) for s in range(0, 8 * 4096, 4096)]


@pytest.mark.usefixtures("small_banks")
def test_the_pure_sawtooth_is_not_windowed(monkeypatch):
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS_ANY_ROOT", True)
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "pure", "sawtooth")
    banked = build(spec)
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(banked)
    r.start()
    got = []
    for s, n in STREAM:
        got.append(banked.render(s, n).data.copy())
        assert banked._bank and banked._bank.request_dependent and banked._bank.win is None
    r.stop()
    plain = build(spec)
    plain._bank = False
    _assert_equal(got, _render_blocks(plain, STREAM), "pure sawtooth stream")
    whole = _render_blocks(build(spec), [(0, 8 * 4096)])[0]
    assert np.max(np.abs(np.concatenate(got).astype(np.float64) - whole)) > 1e-3      # the partition dependence is real and kept


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
def test_a_stateful_bank_is_windowed_and_equals_the_block_by_block_render(monkeypatch, wave):
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "duty", wave)
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS_ANY_ROOT", True)
    banked = build(spec)
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(banked)
    r.start()
    got, opened = [], 0
    for s, n in STREAM:
        got.append(banked.render(s, n).data.copy())
        opened += banked._bank.win is not None
    r.stop()
    assert opened > 0 and not banked._bank.request_dependent
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS_ANY_ROOT", False)
    by_block = build(spec)
    want = _render_blocks(by_block, STREAM)
    assert by_block._bank
    _assert_equal(got, want, "windows")
    plain = build(spec)
    plain._bank = False
    _assert_equal(want, _render_blocks(plain, STREAM), "per-voice path")


# ---------------------------------------------------------------------------------------- 4. the levels above
def _gain(i, osc):
    return S("GainPE", source=osc, gain=_envelope(i + 11))


def _biquad(i, osc):
    return S("BiquadPE", source=osc, frequency=1500.0, q=0.9)


def _ladder(i, osc):
    return S("LadderPE", source=osc, frequency=1200.0, resonance=0.3)


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("form,wave", [("pure", "rectangle"), ("duty", "rectangle"), ("both", "sawtooth")])
@pytest.mark.parametrize("above,node", [(_gain, "_GainNode"), (_biquad, "_BiquadNode"), (_ladder, "_LadderNode")])
def test_levels_above_take_the_new_source(above, node, form, wave):
    banked, got, want, _ = _both_paths(_mix_spec(5, form, wave, above=above))
    root = banked._bank.root
    assert type(root).__name__ == node and isinstance(root.children["source"], voice_bank._AnalogOscNode)
    if above is _ladder:
        # the tolerance test_c4_bank_supersaw_ladder grants the ladder bank
        for a, b in zip(got, want):
            assert float(np.max(np.abs(a.astype(np.float64) - b))) <= 1e-6 * float(np.max(np.abs(b)))
    else:
        _assert_equal(got, want, node)


# ---------------------------------------------------------------------------------------- 5. the oracle
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("form,wave", [("duty", "rectangle"), ("freq", "rectangle"), ("duty", "sawtooth"),
                                       ("freq", "sawtooth"), ("pure", "rectangle")])
def test_bank_against_the_oracle(form, wave):
    spec = _mix_spec(5, form, wave)
    if form != "pure":
        assert osc_edge_distance({"graph": spec, "sr": SR, "blocks": BLOCKS}) > 1e-9
    pg.set_sample_rate(SR)
    banked = build(spec)
    got = _render_blocks(banked)
    assert banked._bank
    oracle = Node(spec, SR)
    for (s, n), g in zip(BLOCKS, got):
        w = oracle.render(s, n)
        assert g.shape == w.shape
        assert np.max(np.abs(g.astype(np.float64) - w)) <= 1e-5 * np.max(np.abs(w)) + 1e-7, (s, n)


# ---------------------------------------------------------------------------------------- 6. fallbacks stay fallbacks
def _lfo_pe(i):
    return pg.TransformPE(pg.SinePE(frequency=0.7 + 0.31 * i), func=pg.transforms.Affine(0.4, 0.5))


def _mixed_waveforms():
    return pg.MixPE(*[pg.AnalogOscPE(_freq(i), _lfo_pe(i), "sawtooth" if i == 2 else "rectangle") for i in range(5)])


def _three_voices():
    return pg.MixPE(*[pg.AnalogOscPE(_freq(i), _lfo_pe(i)) for i in range(3)])


def _shared_lfo():
    lfo = _lfo_pe(0)
    return pg.MixPE(*[pg.AnalogOscPE(_freq(i), lfo) for i in range(5)])


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("make", [_mixed_waveforms, _three_voices, _shared_lfo])
def test_fallbacks_stay_fallbacks(make):
    pg.set_sample_rate(SR)
    mix = make()
    got = _render_blocks(mix)
    assert mix._bank is False
    twin = make()
    twin._bank = False
    _assert_equal(got, _render_blocks(twin), make.__name__)


def test_below_the_measured_minimum_the_voices_are_rendered_one_by_one():
    """No `small_banks`: five such voices are below voice_bank.ANALOG_OSC_MIN_VOICES, where the per-voice path's
    look-ahead windows beat a bank rendered block by block ("AnalogOscPE bank")."""
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "duty", "rectangle", above=_gain)
    mix = build(spec)
    got = _render_blocks(mix)
    assert mix._bank is False
    twin = build(spec)
    twin._bank = False
    _assert_equal(got, _render_blocks(twin), "below the minimum")
