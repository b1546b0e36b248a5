"""GPU: a MixPE of swept-filter voices -- BiquadPE over a BlitSawPE, cutoff and / or Q driven by TransformPE modulators --
is rendered as a voice bank (voice_bank._BiquadVarNode: pgx_biquad_varying_bank) and gives the samples of the per-voice
path bit for bit: the PE's own kernel with the voice in the grid, the same tiles and segments, the same mix order.

Block lengths around the filter's tile of 1024 frames and its plans (tests/channel_cases.py: one workgroup walks up to
two tiles, segments of one tile from three tiles on, of two tiles above 128): a partial fourth segment, exactly one
tile, one frame (the n == 1 state rule), a two-tile walk with a partial tile, a third segment of one frame, a seek;
once 132 099 frames (130 tiles: two per segment, three frames in the last).  4 (voice_bank.MIN_VOICES) and 5 voices, 1,
2 and 3 channels; voice i has mode i % 8 and gain_db in {-3, 0, 3}, so every RBJ branch runs in one launch.

The small banks set voice_bank.BIQUAD_VAR_MIN_VOICES to MIN_VOICES (`small_banks`), as the tests of the other banks set
theirs; one case runs under the measured default.  With the walk (BIQUAD_VAR_WALK_MIN_ROWS rows and more: one workgroup
per row, no segments) and in windows the same float64 recurrence is evaluated in another association: at these Q a
float64 difference is many orders below a float32 ulp, so a sample can at most round the other way -- 6e-8 of its
magnitude against fixture_harness.PEAK_BOUND = 1e-6 of the peak."""

import functools

import numpy as np
import pytest

import pygmu2_amd as pg
from fixture_harness import ABS_FLOOR, PEAK_BOUND, REL_TOL, assert_peak, assert_per_block
from guarded_alloc import guarded
from oracle.golden_cases import S
from oracle.graph_eval import Node
from pygmu2_amd import voice_bank
from pygmu2_amd.biquad_pe import BiquadMode
from spec_build import build

pytestmark = pytest.mark.gpu

SR = 48000
BLOCKS = [(0, 3077), (3077, 1024), (4101, 1), (4102, 2047), (6149, 2049), (30000, 3077)]
LONG = [(0, 132_099)]
FORMS = ("freq", "q", "both")
MODES = [m.value for m in BiquadMode]
NEVER = 1 << 40


@pytest.fixture
def small_banks(monkeypatch):
    monkeypatch.setattr(voice_bank, "BIQUAD_VAR_MIN_VOICES", voice_bank.MIN_VOICES)


@pytest.fixture
def no_walk(monkeypatch):
    monkeypatch.setattr(voice_bank, "BIQUAD_VAR_WALK_MIN_ROWS", NEVER)


def _envelope(i):
    return S("AdsrGatedPE", gate=S("PeriodicGate", frequency=3.0 + 0.17 * i, duty_cycle=0.5),
             attack_time=0.01, decay_time=0.05, sustain_level=0.6, release_time=0.03)


def _cutoff(i):
    return S("TransformPE", source=_envelope(i), ops=[["affine", 2500.0, 300.0 + 40.0 * i]])


def _q(i):
    return S("TransformPE", source=S("SinePE", frequency=0.7 + 0.31 * i), ops=[["affine", 1.2, 2.0]])


def _voice(i, form, channels=1):
    return S("BiquadPE", source=S("BlitSawPE", frequency=109.37 * 2 ** (i / 12), channels=channels),
             frequency=_cutoff(i) if form in ("freq", "both") else 1500.0,
             q=_q(i) if form in ("q", "both") else 2.0, mode=MODES[i % 8], gain_db=3.0 * (i % 3) - 3.0)


def _under_gain(i, form, channels=1):
    return S("GainPE", source=_voice(i, form, channels), gain=_envelope(i + 11))


def _mix_spec(count, form, channels=1, voice=_voice):
    return S("MixPE", inputs=[voice(i % 64, form, channels) for i in range(count)])


def _render_blocks(root, blocks=BLOCKS):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(root)
    r.start()
    out = [root.render(s, n).data.copy() for s, n in blocks]
    r.stop()
    return out


def _both_paths(spec, blocks=BLOCKS):
    """(the banked MixPE, its blocks, the blocks of a twin rendered voice by voice)"""
    pg.set_sample_rate(SR)
    banked = build(spec)
    got = _render_blocks(banked, blocks)
    assert banked._bank, "no voice bank was built"
    plain = build(spec)
    plain._bank = False
    return banked, got, _render_blocks(plain, blocks)


def _assert_equal(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        assert np.any(b), f"{what} block {k} is silent"
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{what} block {k}: max|d| = {np.max(np.abs(a.astype(np.float64) - b))}"


def _var_node(bank):
    node = bank.root
    while not isinstance(node, voice_bank._BiquadVarNode):
        node = node.children["source"]
    return node


def _check_tree(bank, count, form):
    node = _var_node(bank)
    assert node.k == count and not isinstance(node, voice_bank._BiquadNode)
    assert set(node.children) == {"source"} | ({"frequency"} if form != "q" else set()) | ({"q"} if form != "freq" else set())
    assert isinstance(node.children["source"], voice_bank._BlitSawNode)
    for name in ("frequency", "q"):
        if name in node.children:
            assert isinstance(node.children[name], voice_bank._TransformNode) and node.children[name].channels() == 1
    return node


# ---------------------------------------------------------------------------------------- 1. the per-voice path, bit for bit
@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_bank_equals_the_per_voice_path(form, channels):
    with guarded():
        for count in (4, 5):
            banked, got, want = _both_paths(_mix_spec(count, form, channels))
            node = _check_tree(banked._bank, count, form)
            assert banked._bank.root is node
            assert got[0].shape == (BLOCKS[0][1], channels)
            _assert_equal(got, want, f"{form} x{count} ch={channels}")
            assert node.state.shape == (count, channels, 4)


@pytest.mark.usefixtures("small_banks", "no_walk")
def test_the_long_block_two_tiles_per_segment():
    with guarded():
        banked, got, want = _both_paths(_mix_spec(4, "both"), LONG)
        _check_tree(banked._bank, 4, "both")
        _assert_equal(got, want, "132 099 frames")


@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("form", FORMS)
def test_voices_under_an_envelope_gain(form):
    """GainPE(<voice>, gain=AdsrGatedPE): the two-stream branch of VoiceBank._render_mix_now."""
    with guarded():
        banked, got, want = _both_paths(_mix_spec(5, form, voice=_under_gain))
        root = banked._bank.root
        assert isinstance(root, voice_bank._GainNode) and isinstance(root.children["gain"], voice_bank._AdsrGatedNode)
        assert root.children["source"] is _check_tree(banked._bank, 5, form)
        _assert_equal(got, want, f"gain {form}")


@pytest.mark.usefixtures("no_walk")
def test_under_the_measured_minimum():
    """No `small_banks`: 70 voices, or the measured minimum where that is more."""
    count = max(70, voice_bank.BIQUAD_VAR_MIN_VOICES)
    assert voice_bank.MIN_VOICES <= voice_bank.BIQUAD_VAR_MIN_VOICES <= count
    with guarded():
        banked, got, want = _both_paths(_mix_spec(count, "both", voice=_under_gain), BLOCKS[:3] + BLOCKS[-1:])
        assert _var_node(banked._bank).k == count
        _assert_equal(got, want, f"{count} voices")
        if voice_bank.BIQUAD_VAR_MIN_VOICES > voice_bank.MIN_VOICES:
            pg.set_sample_rate(SR)
            below = build(_mix_spec(voice_bank.BIQUAD_VAR_MIN_VOICES - 1, "both", voice=_under_gain))
            _render_blocks(below, BLOCKS[2:3])
            assert below._bank is False


# ---------------------------------------------------------------------------------------- 2. the walk
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_the_walk_stays_within_a_rounding_of_the_per_voice_path(monkeypatch, form, channels):
    monkeypatch.setattr(voice_bank, "BIQUAD_VAR_WALK_MIN_ROWS", 1)
    with guarded():
        banked, got, want = _both_paths(_mix_spec(5, form, channels))
        node = _check_tree(banked._bank, 5, form)
        assert node.ws is None                               # no workspace: one workgroup per row
        assert_peak(f"walk {form} ch={channels}", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "WALK")


# ---------------------------------------------------------------------------------------- 3. lifecycle
@pytest.mark.usefixtures("small_banks", "no_walk")
def test_stop_start_gives_the_same_samples_again():
    pg.set_sample_rate(SR)
    with guarded():
        banked = build(_mix_spec(5, "both"))
        first = _render_blocks(banked)
        assert banked._bank
        state = _var_node(banked._bank).state
        assert not np.any(state.to_host())                   # stop() has put the filters to rest
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(banked)
        r.start()
        banked.render(*BLOCKS[0])
        assert np.all(np.any(state.to_host() != 0.0, axis=(1, 2)))      # every voice carries {x1, x2, y1, y2}
        r.stop()
        again = _render_blocks(banked)                       # stop / start in between
        assert _var_node(banked._bank).state is state
        _assert_equal(again, first, "stop/start")
        plain = build(_mix_spec(5, "both"))
        plain._bank = False
        _assert_equal(first, _render_blocks(plain), "per-voice path")


@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("voice", [_voice, _under_gain])
def test_windows_snapshot_and_restore_the_filter_state(voice):
    """A rank's share of a sharded mix: windows at the level of the mix.  Six equal pulls (windows of 2 and 4 blocks), then
    a pull back to the second block: the states go back to the window's start and the consumed part is rendered again."""
    pulls = [(s, 4096) for s in range(0, 6 * 4096, 4096)] + [(4096, 4096), (8192, 4096)]
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, "both", voice=voice)
    with guarded():
        banked = build(spec)
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(banked)
        r.start()
        assert banked._voice_bank()
        banked._bank.set_mix_windows()
        got, opened = [], 0
        for s, n in pulls:
            got.append(banked.render(s, n).data.copy())
            opened += banked._bank.win is not None
        r.stop()
        assert opened >= 2
        by_block = build(spec)
        want = _render_blocks(by_block, pulls)
        assert by_block._bank
        assert_peak(f"windows {voice.__name__}", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "WINDOWS")


# ---------------------------------------------------------------------------------------- 4. the oracle
@functools.lru_cache(maxsize=None)
def _oracle_blocks(form, long):
    spec = _mix_spec(4 if long else 5, form)
    oracle = Node(spec, SR)
    blocks = LONG if long else BLOCKS
    out = [oracle.render(s, n) for s, n in blocks]
    for block in out:
        block.setflags(write=False)
    return out


@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("form,long", [("freq", False), ("q", False), ("both", False), ("both", True)])
def test_bank_against_the_oracle(form, long):
    want = _oracle_blocks(form, long)
    assert all(float(np.max(np.abs(w))) > 1e-3 for w in want)            # (not silent)
    blocks = LONG if long else BLOCKS
    pg.set_sample_rate(SR)
    with guarded():
        banked = build(_mix_spec(4 if long else 5, form))
        got = _render_blocks(banked, blocks)
        assert banked._bank
    assert_per_block(f"oracle {form}", got, dict(enumerate(want)), REL_TOL, ABS_FLOOR, "ORACLE")

