"""GPU: a MixPE of percussive voices -- SVFilterPE over a BlitSawPE, AdsrTriggeredPE(PeriodicTrigger) as a gain or a cutoff
envelope -- is rendered as a voice bank (voice_bank._SvfNode: pgx_svf_bank; _TriggerNode: pgx_periodic_trigger_bank;
_AdsrTriggeredNode: pgx_adsr_triggered with batch = K) and gives the samples of the per-voice path bit for bit: the PEs'
own kernels with the voice in the grid, the same tiles and segments, the same mix order.

Block lengths around the filter's tile of 1024 frames and its plans (tests/channel_cases.py): a partial fourth segment,
exactly one tile, one frame, a two-tile walk with a partial tile, a third segment of one frame, a seek.  4
(voice_bank.MIN_VOICES) and 5 voices, 1 and 2 channels; voice i has SVF mode i % 7 and gain_db in {-3, 0, 3}.  The small
banks set the measured minimums to MIN_VOICES (`small_banks`) and keep the segmented plan (`no_walk`).

Where the same float64 recurrence is evaluated in another association -- the bank's windows of several blocks, the
on-chip mix of BiquadPE voices -- a sample can at most round the other way: fixture_harness.PEAK_BOUND = 1e-6 of the
peak, the bound tests/test_gpu_swept_bank.py and tests/test_gpu_voice_tiles.py hold those paths to."""

import functools

import numpy as np
import pytest

import pygmu2_amd as pg
from fixture_harness import PEAK_BOUND, assert_peak
from guarded_alloc import guarded
from oracle.golden_cases import S
from oracle.graph_eval import Node
from pygmu2_amd import voice_bank
from spec_build import build

pytestmark = pytest.mark.gpu

SR = 48000
BLOCKS = [(0, 3077), (3077, 1024), (4101, 1), (4102, 2047), (6149, 2049), (30000, 3077)]
SVF_MODES = ["lowpass", "highpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf"]
NEVER = 1 << 40


@pytest.fixture
def small_banks(monkeypatch):
    for name in ("SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES", "BIQUAD_VAR_MIN_VOICES"):
        monkeypatch.setattr(voice_bank, name, voice_bank.MIN_VOICES)


@pytest.fixture
def no_walk(monkeypatch):
    monkeypatch.setattr(voice_bank, "SVF_WALK_MIN_ROWS", NEVER)
    monkeypatch.setattr(voice_bank, "BIQUAD_VAR_WALK_MIN_ROWS", NEVER)


def _saw(i, channels=1):
    return S("BlitSawPE", frequency=109.37 * 2 ** ((i % 64) / 12), channels=channels)


def _envelope(i):
    """A hit every 1 / (3 + 0.17 i) s: 5 ms attack, 40 ms decay, 50 ms at 0.6, 80 ms release (silent before the next)."""
    return S("AdsrTriggeredPE", trigger=S("PeriodicTrigger", hz=3.0 + 0.17 * i), attack_time=0.005, decay_time=0.04,
             sustain_time=0.05, sustain_level=0.6, release_time=0.08)


def _svf(i, channels=1):
    return S("SVFilterPE", source=_saw(i, channels), frequency=1200.0 + 40.0 * i, q=2.0 + 0.1 * i, mode=SVF_MODES[i % 7],
             gain_db=3.0 * (i % 3) - 3.0)


def _svf_under_envelope(i, channels=1):
    return S("GainPE", source=_svf(i, channels), gain=_envelope(i))


def _swept_under_envelope(i, channels=1):
    cutoff = S("TransformPE", source=_envelope(i + 7), ops=[["affine", 2500.0, 300.0 + 40.0 * i]])
    return S("GainPE", source=S("BiquadPE", source=_saw(i, channels), frequency=cutoff, q=2.0), gain=_envelope(i))


def _biquad_under_envelope(i, channels=1):
    return S("GainPE", source=S("BiquadPE", source=S("BlitSawPE", frequency=27.5 * 2 ** ((i % 16) / 4.0)), frequency=2000.0,
                                q=0.707), gain=_envelope(i))


def _mix_spec(count, voice, channels=1):
    return S("MixPE", inputs=[voice(i, channels) for i in range(count)])


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
        assert np.all(np.isfinite(b)) and np.any(b), f"{what} block {k} is silent"
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"{what} block {k}: max|d| = {np.max(np.abs(a.astype(np.float64) - b))}"


def _check_envelope(node, count):
    assert type(node) is voice_bank._AdsrTriggeredNode and node.k == count
    assert not isinstance(node, voice_bank._AdsrGatedNode)
    assert node.state.shape == (count, 3)
    trigger = node.children["trigger"]
    assert type(trigger) is voice_bank._TriggerNode and trigger.k == count


def _check_svf(node, count, channels):
    assert type(node) is voice_bank._SvfNode and node.k == count
    assert isinstance(node.children["source"], voice_bank._BlitSawNode)
    assert node.state.shape == (count, channels, 2)
    assert node.ws is not None                                       # the segmented plan, as the PE
    return node


# ---------------------------------------------------------------------------------------- (a) SVF voices, bit for bit
@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("channels", [1, 2])
def test_svf_voices_equal_the_per_voice_path(channels):
    with guarded():
        for count in (4, 5):
            banked, got, want = _both_paths(_mix_spec(count, _svf, channels))
            _check_svf(banked._bank.root, count, channels)
            assert got[0].shape == (BLOCKS[0][1], channels)
            _assert_equal(got, want, f"svf x{count} ch={channels}")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("channels", [1, 2])
def test_the_walk_stays_within_a_rounding_of_the_per_voice_path(monkeypatch, channels):
    """From SVF_WALK_MIN_ROWS rows on the node passes no workspace: one workgroup per row, the same float64 scan in
    another association."""
    monkeypatch.setattr(voice_bank, "SVF_WALK_MIN_ROWS", 1)
    with guarded():
        banked, got, want = _both_paths(_mix_spec(5, _svf, channels))
        node = banked._bank.root
        assert type(node) is voice_bank._SvfNode and node.k == 5 and node.ws is None
        assert_peak(f"walk ch={channels}", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "WALK")


# ---------------------------------------------------------------------------------------- (b) ... under a triggered envelope
@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("channels", [1, 2])
def test_svf_voices_under_a_triggered_envelope(channels):
    with guarded():
        for count in (4, 5):
            banked, got, want = _both_paths(_mix_spec(count, _svf_under_envelope, channels))
            root = banked._bank.root
            assert type(root) is voice_bank._GainNode and root.k == count
            _check_svf(root.children["source"], count, channels)
            _check_envelope(root.children["gain"], count)
            _assert_equal(got, want, f"svf x envelope x{count} ch={channels}")


# ---------------------------------------------------------------------------------------- (c) the envelope sweeps a biquad
@pytest.mark.usefixtures("small_banks", "no_walk")
@pytest.mark.parametrize("channels", [1, 2])
def test_a_triggered_envelope_drives_a_swept_biquad(channels):
    with guarded():
        for count in (4, 5):
            banked, got, want = _both_paths(_mix_spec(count, _swept_under_envelope, channels))
            root = banked._bank.root
            assert type(root) is voice_bank._GainNode and root.k == count
            _check_envelope(root.children["gain"], count)
            swept = root.children["source"]
            assert type(swept) is voice_bank._BiquadVarNode and swept.k == count and set(swept.children) == {"source", "frequency"}
            cutoff = swept.children["frequency"]
            assert type(cutoff) is voice_bank._TransformNode
            _check_envelope(cutoff.children["source"], count)
            _assert_equal(got, want, f"swept x{count} ch={channels}")


# ---------------------------------------------------------------------------------------- (d) the on-chip mix
def test_sixteen_biquad_voices_under_triggered_envelopes_mix_on_chip(monkeypatch):
    """GainPE(BiquadPE(BlitSawPE), gain=AdsrTriggeredPE): from VOICE_TILES_MIN_VOICES voices and 4096 frames on the bank
    mixes on chip (pgx_voice_tiles), in windows, and takes the triggered envelopes' rows as it takes any gain rows --
    rendered on the main stream, none of the gated envelope's run-ahead.  tests/test_gpu_voice_tiles.py's bound."""
    monkeypatch.setattr(voice_bank, "ADSR_TRIGGERED_MIN_VOICES", voice_bank.MIN_VOICES)
    assert voice_bank.VOICE_TILES_MIN_VOICES <= 16
    blocks = [(s, 4096) for s in range(0, 7 * 4096, 4096)] + [(4096, 4096), (8192, 4096), (100_000, 4099)]
    with guarded():
        banked, got, want = _both_paths(_mix_spec(16, _biquad_under_envelope), blocks)
        root = banked._bank.root
        assert type(root) is voice_bank._GainNode and root.k == 16
        _check_envelope(root.children["gain"], 16)
        assert type(root.children["source"]) is voice_bank._BiquadNode
        assert banked._bank._mixes_on_chip(4096)
        peak = max(float(np.max(np.abs(b))) for b in want)
        assert peak > 1e-3
        for (s, n), a, b in zip(blocks, got, want):
            assert a.shape == b.shape == (n, 1) and np.any(b)
            err = float(np.max(np.abs(a - b)))
            print(f"ONCHIP block {(s, n)} max_abs_err={err:.3e} peak={peak:.3e}")
            assert err <= 1e-6 * peak, f"block {(s, n)}: {err / peak:.3e} of peak"


# ---------------------------------------------------------------------------------------- the measured minimums
@pytest.mark.parametrize("voice,constant", [(_svf, "SVF_MIN_VOICES"), (_biquad_under_envelope, "ADSR_TRIGGERED_MIN_VOICES")])
def test_under_the_measured_minimums(voice, constant):
    """No `small_banks`, no `no_walk`: the bank as it is built by default -- at the measured minimum (the SVF bank walks
    from SVF_WALK_MIN_ROWS rows on, short blocks keep the layered path under the envelopes) --, and none one voice below."""
    count = getattr(voice_bank, constant)
    assert voice_bank.MIN_VOICES <= count <= 1024
    blocks = BLOCKS[:3] + BLOCKS[-1:]
    with guarded():
        banked, got, want = _both_paths(_mix_spec(count, voice), blocks)
        assert banked._bank.k == count
        assert_peak(f"{count} voices", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "DEFAULT")
        if count > voice_bank.MIN_VOICES:
            pg.set_sample_rate(SR)
            below = build(_mix_spec(count - 1, voice))
            _render_blocks(below, BLOCKS[2:3])
            assert below._bank is False


# ---------------------------------------------------------------------------------------- (e) the oracle
@functools.lru_cache(maxsize=None)
def _oracle_blocks():
    oracle = Node(_mix_spec(5, _svf_under_envelope), SR)
    out = [oracle.render(s, n) for s, n in BLOCKS]
    for block in out:
        block.setflags(write=False)
    return out


@pytest.mark.usefixtures("small_banks", "no_walk")
def test_bank_against_the_oracle():
    want = _oracle_blocks()
    assert all(float(np.max(np.abs(w))) > 1e-3 for w in want[:2])         # (not silent)
    pg.set_sample_rate(SR)
    with guarded():
        banked = build(_mix_spec(5, _svf_under_envelope))
        got = _render_blocks(banked)
        assert banked._bank and type(banked._bank.root.children["source"]) is voice_bank._SvfNode
    assert_peak("oracle svf x envelope", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "ORACLE")


# ---------------------------------------------------------------------------------------- (f) windows
@pytest.mark.usefixtures("small_banks", "no_walk")
def test_equal_blocks_in_windows_stay_within_a_rounding_of_the_per_voice_path():
    """A rank's share of a sharded mix: windows at the level of the mix (BANK_WINDOWS).  Six equal pulls (windows of 2 and
    4 blocks), then a pull back to the second block: every node's state -- the filters' {s0, s1}, the envelopes' {state,
    level, deadline} -- goes back to the window's start and the consumed part is rendered again.  A window is one long
    block to the filter: the same float64 scan in another association."""
    pulls = [(s, 4096) for s in range(0, 6 * 4096, 4096)] + [(4096, 4096), (8192, 4096)]
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, _svf_under_envelope)
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
        _check_envelope(banked._bank.root.children["gain"], 5)
        plain = build(spec)
        plain._bank = False
        want = _render_blocks(plain, pulls)
    assert_peak("windows svf x envelope", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "WINDOWS")


# ---------------------------------------------------------------------------------------- (g) lifecycle
@pytest.mark.usefixtures("small_banks", "no_walk")
def test_a_seek_backwards_and_stop_start_give_the_per_voice_samples_again():
    blocks = BLOCKS + [(3077, 1024), (4101, 2047)]                   # ... and back into the stream
    pg.set_sample_rate(SR)
    spec = _mix_spec(5, _svf_under_envelope, 2)
    with guarded():
        banked = build(spec)
        first = _render_blocks(banked, blocks)
        assert banked._bank
        root = banked._bank.root
        svf, envelope = _check_svf(root.children["source"], 5, 2), root.children["gain"]
        _check_envelope(envelope, 5)
        svf_state, envelope_state = svf.state, envelope.state
        assert not np.any(svf_state.to_host()) and not np.any(envelope_state.to_host())     # stop() has put them to rest
        r = pg.NullRenderer(sample_rate=SR)
        r.set_source(banked)
        r.start()
        banked.render(*BLOCKS[0])
        assert np.all(np.any(svf_state.to_host() != 0.0, axis=(1, 2)))       # every voice carries {s0, s1}
        assert np.all(envelope_state.to_host()[:, 2] > 0.0)                  # ... and a sustain deadline
        r.stop()
        again = _render_blocks(banked, blocks)                               # stop / start in between
        assert svf.state is svf_state and envelope.state is envelope_state
        _assert_equal(again, first, "stop/start")
        plain = build(spec)
        plain._bank = False
        _assert_equal(first, _render_blocks(plain, blocks), "per-voice path")
