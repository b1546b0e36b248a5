"""GPU: a MixPE of NoisePE voices is rendered as a voice bank (voice_bank._NoiseNode: pgx_noise_white / _pink / _brown with
batch = K) and gives, sample for sample (np.array_equal), (a) the float32 sum in voice order of the streams of the numpy
restatement (tests/noise_oracle.NoiseStream) and (b) what a twin graph rendered voice by voice (`mix._bank = False`) gives.
Also: hi-hat voices -- GainPE(SVFilterPE(NoisePE), gain=AdsrTriggeredPE(PeriodicTrigger)) --, and AnalogOscPE / BiquadPE
voices whose duty cycle / cutoff follows a FunctionGenPE (voice_bank._FunctionGenNode: pgx_function_gen_bank), against
the per-voice path at the bar tests/test_gpu_analog_bank.py (np.array_equal, its _assert_equal) and
tests/test_gpu_swept_bank.py (bit for bit, with the segmented plan) hold the same trees to under a SinePE modulator.

A noise stream does not depend on how it is cut, and `start` is ignored: the oracle's stream of voice i is computed once
per (mode, voice) and a pull pattern takes consecutive pieces of it.  Patterns: one block of 2 049 frames; blocks of 256;
blocks of 1, 1 023, 1 025, 2 047, 2 049 (across the kernels' tiles of 1 024 and 2 048 frames); a seek back and a gap (the
stream goes on); 4 096-frame blocks in windows of the mix with a seek in the middle of a window (the stream is where
the consumed blocks left it); reset_state() of every voice and renderer stop / start (the stream starts over).  5 and 65
voices, default and scaled ranges within one bank.  The measured minimums are set to MIN_VOICES (`small_banks`)."""

import functools

import numpy as np
import pytest

import noise_oracle as P
import pygmu2_amd as pg
from fixture_harness import PEAK_BOUND, assert_peak
from guarded_alloc import guarded
from pygmu2_amd import look_ahead, voice_bank
from pygmu2_amd.biquad_pe import BiquadMode
from pygmu2_amd.transforms import Affine

pytestmark = pytest.mark.gpu

SR = 48000
MODES = {"white": pg.NoiseMode.WHITE, "pink": pg.NoiseMode.PINK, "brown": pg.NoiseMode.BROWN}
ENTRY = {"white": "pgx_noise_white", "pink": "pgx_noise_pink", "brown": "pgx_noise_brown"}
ONE = [(0, 2049)]
SMALL = [(256 * i, 256) for i in range(6)]
ODD = [(0, 1), (1, 1023), (1024, 1025), (2049, 2047), (4096, 2049)]
SEEK = [(0, 1024), (1024, 1024), (512, 1024), (10_000, 1024)]
STREAM = [(4096 * i, 4096) for i in range(5)] + [(4096, 4096), (8192, 4096)]     # windows of 2 and 4; a seek after 2 of the 4
PATTERNS = {"one": ONE, "small": SMALL, "odd": ODD, "seek": SEEK}
SHORT, LONG = 6400, 7 * 4096                      # frames of oracle stream: every pattern but STREAM; STREAM (5 voices)


@pytest.fixture
def small_banks(monkeypatch):
    for name in ("NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES", "ANALOG_OSC_MIN_VOICES",
                 "BIQUAD_VAR_MIN_VOICES"):
        monkeypatch.setattr(voice_bank, name, voice_bank.MIN_VOICES)
    monkeypatch.setattr(voice_bank, "BIQUAD_VAR_WALK_MIN_ROWS", 1 << 40)


def _range(i):
    """Every third voice draws in the default range (the draw passes untouched), the others are scaled."""
    return (-1.0, 1.0) if i % 3 == 0 else (-0.5 + 0.125 * (i % 4), 0.75 + 0.25 * (i % 5))


def _noise(i, mode):
    lo, hi = _range(i)
    return pg.NoisePE(lo, hi, seed=100 + i, mode=MODES[mode])


def _noise_mix(count, mode, bank=True):
    mix = pg.MixPE(*[_noise(i, mode) for i in range(count)])
    if not bank:
        mix._bank = False
    return mix


@functools.lru_cache(maxsize=None)
def _stream(mode, i, frames, skip_at=None, skip=0):
    """The first `frames` samples voice i renders (skip_at: `skip` draws are passed over after that many frames)."""
    lo, hi = _range(i)
    s = P.NoiseStream(100 + i, mode, lo, hi)
    if skip_at is None:
        out = s.render(frames)[:, 0]
    else:
        head = s.render(skip_at)[:, 0]
        s.rng.bit_generator.advance(skip)
        out = np.concatenate([head, s.render(frames - skip_at)[:, 0]])
    out.setflags(write=False)
    return out


def _mixed(streams, at, n):
    """MixPE's sum: float32, in voice order."""
    acc = streams[0][at:at + n].copy()
    for s in streams[1:]:
        acc = acc + s[at:at + n]
    assert acc.dtype == np.float32
    return acc.reshape(-1, 1)


def _expected(mode, count, blocks, frames, restart_at=(), **skip):
    """The blocks a stream of consecutive pieces gives; restart_at: block indices in front of which the stream starts over."""
    streams = [_stream(mode, i, frames, *((skip["at"], skip["draws"]) if skip.get("voice") == i else ())) for i in range(count)]
    out, at = [], 0
    for k, (_, n) in enumerate(blocks):
        if k in restart_at:
            at = 0
        out.append(_mixed(streams, at, n))
        at += n
    assert at <= frames
    return out


def _started(root):
    r = pg.NullRenderer(sample_rate=SR)
    r.set_source(root)
    r.start()
    return r


def _render_blocks(root, blocks, between=None):
    """between: {block index: function called in front of that block}"""
    r = _started(root)
    out = []
    for k, (s, n) in enumerate(blocks):
        if between and k in between:
            between[k]()
        out.append(root.render(s, n).data.copy())
    r.stop()
    return out


def _assert_equal(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, f"{what} block {k}: {a.shape} {b.shape}"
        assert np.all(np.isfinite(b)) and np.any(b), f"{what} block {k} is silent"
        assert np.array_equal(a, b), f"{what} block {k}: max|d| = {np.max(np.abs(a.astype(np.float64) - b))}"


def _node(mix, count, mode):
    node = mix._bank.root
    assert type(node) is voice_bank._NoiseNode and node.k == count and node.entry == ENTRY[mode]
    assert (node.state is None) == (mode == "white")
    return node


# ---------------------------------------------------------------------------------------- 1. oracle and per-voice path
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("windows", [True, False])
@pytest.mark.parametrize("count", [5, 65])
@pytest.mark.parametrize("mode", list(MODES))
def test_bank_equals_the_oracle_and_the_per_voice_path(monkeypatch, mode, count, windows):
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS", windows)
    pg.set_sample_rate(SR)
    with guarded():
        for name, blocks in PATTERNS.items():
            what = f"{mode} x{count} {name} windows={windows}"
            banked = _noise_mix(count, mode)
            got = _render_blocks(banked, blocks)
            node = _node(banked, count, mode)
            assert node.draws == 0                                       # (stop() has reset the bank)
            _assert_equal(got, _expected(mode, count, blocks, SHORT), what + ": oracle")
            _assert_equal(got, _render_blocks(_noise_mix(count, mode, bank=False), blocks), what + ": per voice")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("windows", [True, False])
@pytest.mark.parametrize("mode", list(MODES))
def test_a_seek_in_the_middle_of_a_window(monkeypatch, mode, windows):
    """Windows at the level of the mix (a rank's share of a sharded mix): five equal pulls open windows of 2 and of 4
    blocks; the pull back leaves the second window after two of them.  The stream goes on where the consumed blocks ended."""
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS", windows)
    pg.set_sample_rate(SR)
    with guarded():
        banked = _noise_mix(5, mode)
        r = _started(banked)
        assert banked._voice_bank()
        banked._bank.set_mix_windows()
        got, opened = [], 0
        for s, n in STREAM:
            got.append(banked.render(s, n).data.copy())
            opened += banked._bank.win is not None
        assert _node(banked, 5, mode).draws >= 7 * 4096              # (what was consumed; a window may have run ahead)
        assert windows or banked._bank.root.draws == 7 * 4096
        r.stop()
        assert (opened >= 3) if windows else (opened == 0)
        _assert_equal(got, _expected(mode, 5, STREAM, LONG), f"{mode} windows={windows}: oracle")
        _assert_equal(got, _render_blocks(_noise_mix(5, mode, bank=False), STREAM), f"{mode} windows={windows}: per voice")


# ---------------------------------------------------------------------------------------- 2. lifecycle
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("mode", list(MODES))
def test_reset_state_and_stop_start_restart_the_stream(mode):
    pg.set_sample_rate(SR)
    blocks = ODD + [(0, 1), (1, 1023)]

    def reset_all(mix):
        return lambda: [pe.reset_state() for pe in mix.inputs()]

    with guarded():
        banked = _noise_mix(5, mode)
        first = _render_blocks(banked, blocks, {5: reset_all(banked)})
        node = _node(banked, 5, mode)
        want = _expected(mode, 5, blocks, SHORT, restart_at=(5,))
        _assert_equal(first, want, f"{mode}: reset_state of every voice")
        _assert_equal(first[5:], first[:2], f"{mode}: the stream started over")
        again = _render_blocks(banked, blocks, {5: reset_all(banked)})       # stop / start in between: the same bank
        assert banked._bank.root is node
        _assert_equal(again, first, f"{mode}: stop / start")
        plain = _noise_mix(5, mode, bank=False)
        _assert_equal(first, _render_blocks(plain, blocks, {5: reset_all(plain)}), f"{mode}: per voice")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("mode", list(MODES))
def test_reset_state_of_one_voice_restarts_that_voice_alone(mode):
    pg.set_sample_rate(SR)
    blocks = [(0, 1500), (1500, 1500)]
    with guarded():
        banked = _noise_mix(5, mode)
        got = _render_blocks(banked, blocks, {1: banked.inputs()[3].reset_state})
        streams = [_stream(mode, i, SHORT) for i in range(5)]
        second = [s[1500:3000] for s in streams]
        second[3] = streams[3][:1500]
        _assert_equal(got, [_mixed(streams, 0, 1500), _mixed(second, 0, 1500)], f"{mode}: voice 3 reset")
        plain = _noise_mix(5, mode, bank=False)
        _assert_equal(got, _render_blocks(plain, blocks, {1: plain.inputs()[3].reset_state}), f"{mode}: per voice")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("windows", [True, False])
@pytest.mark.parametrize("at", [3, 4])
@pytest.mark.parametrize("who", ["every voice", "voice 3"])
@pytest.mark.parametrize("mode", list(MODES))
def test_reset_state_around_a_window(monkeypatch, mode, who, at, windows):
    """Windows at the level of the mix, seven pulls of 4 096 frames: blocks 0 .. 4 in order (a window of 2 opens at block 1,
    a window of 4 at block 3), then a seek back to frame 4 096 and the block after it.  reset_state() -- of every voice, or
    of voice 3 alone -- in front of block 3 is applied by the very render that opens the window of 4; in front of block 4 it
    finds that window open and settles it.  Either way the seek, which leaves the window half consumed and puts the states
    back to its start, must not undo the reset: the streams go on from where the consumed blocks left them."""
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS", windows)
    pg.set_sample_rate(SR)
    B = 4096
    resetting = range(5) if who == "every voice" else (3,)

    def reset(mix):
        return lambda: [mix.inputs()[i].reset_state() for i in resetting]

    streams = []
    for i in range(5):
        whole = _stream(mode, i, LONG)
        streams.append(np.concatenate([whole[:at * B], whole[:(7 - at) * B]]) if i in resetting else whole)
    want = [_mixed(streams, k * B, B) for k in range(7)]
    with guarded():
        banked = _noise_mix(5, mode)
        r = _started(banked)
        assert banked._voice_bank()
        banked._bank.set_mix_windows()
        got, opened = [], []
        for k, (s, n) in enumerate(STREAM):
            if k == at:
                reset(banked)()
                assert banked._bank.win is None                  # (a window that was open has been settled)
            got.append(banked.render(s, n).data.copy())
            opened.append(banked._bank.win is not None)
        node = _node(banked, 5, mode)
        assert not node.pending
        host, device = node.rec.copy(), node.params.to_host()
        assert host.tobytes() == np.ascontiguousarray(device).tobytes()      # the records the kernel reads are the host's
        r.stop()
        assert opened[3] == windows and opened[5] is False
        _assert_equal(got, want, f"{mode} {who} at {at} windows={windows}: oracle")
        plain = _noise_mix(5, mode, bank=False)
        _assert_equal(got, _render_blocks(plain, STREAM, {at: reset(plain)}), f"{mode} {who} at {at}: per voice")


@pytest.mark.usefixtures("small_banks")
def test_seed_none_draws_fresh_entropy_per_voice_and_per_start():
    pg.set_sample_rate(SR)
    with guarded():
        mix = pg.MixPE(*[pg.NoisePE(seed=None) for _ in range(5)])
        first = _render_blocks(mix, ONE)[0]
        assert mix._bank
        states = {(int(r["state_hi"]), int(r["state_lo"])) for r in mix._bank.root.rec}
        assert len(states) == 5
        again = _render_blocks(mix, ONE)[0]
        assert np.all(np.abs(first) <= 5.0) and not np.array_equal(first, again)


# ---------------------------------------------------------------------------------------- 3. advance
@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("mode", list(MODES))
def test_advance_on_one_voice_skips_that_voice_alone(mode):
    """advance(1000) on voice 2 between two blocks: the oracle's stream of that voice skips 1000 draws there (taps and level
    stay), and the twin rendered voice by voice, block by block, gives the same."""
    pg.set_sample_rate(SR)
    blocks = [(0, 2049), (2049, 1023), (3072, 256)]
    with guarded():
        banked = _noise_mix(5, mode)
        got = _render_blocks(banked, blocks, {1: lambda: banked.inputs()[2].advance(1000)})
        _node(banked, 5, mode)
        want = _expected(mode, 5, blocks, SHORT, voice=2, at=2049, draws=1000)
        _assert_equal(got, want, f"{mode}: advance, oracle")
        assert not np.array_equal(got[1], _expected(mode, 5, blocks, SHORT)[1])
        was = look_ahead.enabled()
        look_ahead.set_enabled(False)
        try:
            plain = _noise_mix(5, mode, bank=False)
            twin = _render_blocks(plain, blocks, {1: lambda: plain.inputs()[2].advance(1000)})
        finally:
            look_ahead.set_enabled(was)
        _assert_equal(got, twin, f"{mode}: advance, per voice")


@pytest.mark.usefixtures("small_banks")
def test_advance_in_the_middle_of_a_window():
    """The bank has run ahead by a window when advance() comes: the window is settled, the voice skips from the last block
    handed out."""
    pg.set_sample_rate(SR)
    blocks = [(4096 * i, 4096) for i in range(6)]
    with guarded():
        banked = _noise_mix(5, "pink")
        r = _started(banked)
        assert banked._voice_bank()
        banked._bank.set_mix_windows()
        got = []
        for k, (s, n) in enumerate(blocks):
            if k == 4:
                assert banked._bank.win is not None              # the window of 4 opened at block 3
                banked.inputs()[2].advance(1000)
                assert banked._bank.win is None
            got.append(banked.render(s, n).data.copy())
        r.stop()
        _assert_equal(got, _expected("pink", 5, blocks, LONG, voice=2, at=4 * 4096, draws=1000), "advance in a window")


# ---------------------------------------------------------------------------------------- 4. the hi-hat bank
HAT_SR = 8000
HAT_PATTERNS = {"stream": [(1024 * i, 1024) for i in range(3)], "seek": [(0, 1024), (1024, 1024), (512, 1024), (3000, 1024)]}


def _hihat(i):
    """A hit every 1 / (4 + 0.5 i) s -- 2 000 frames and less at 8 kHz: hits fall inside the second and third block."""
    envelope = pg.AdsrTriggeredPE(pg.PeriodicTrigger(4.0 + 0.5 * i), 0.001, 0.02, 0.03, 0.3, 0.05)
    return pg.GainPE(pg.SVFilterPE(pg.NoisePE(seed=i), 1500.0 + 150.0 * i, 2.0, BiquadMode.HIGHPASS), gain=envelope)


def _hihat_mix(bank=True):
    mix = pg.MixPE(*[_hihat(i) for i in range(8)])
    if not bank:
        mix._bank = False
    return mix


def _render_hat(root, blocks, ahead=False):
    """Block by block on both paths (look-ahead off: the per-voice filters then run over the same blocks as the bank's --
    pgx_svf_bank is pgx_svf bit for bit at the same block length; a longer look-ahead window is the same recurrence in
    another association).  ahead: look-ahead on, the default configuration."""
    was = look_ahead.enabled()
    look_ahead.set_enabled(ahead)
    try:
        r = pg.NullRenderer(sample_rate=HAT_SR)
        r.set_source(root)
        r.start()
        out = [root.render(s, n).data.copy() for s, n in blocks]
        r.stop()
    finally:
        look_ahead.set_enabled(was)
    return out


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("windows", [True, False])
def test_hihat_voices_equal_the_per_voice_path(monkeypatch, windows):
    monkeypatch.setattr(voice_bank, "BANK_WINDOWS", windows)
    pg.set_sample_rate(HAT_SR)
    try:
        with guarded():
            for name, blocks in HAT_PATTERNS.items():
                banked = _hihat_mix()
                got = _render_hat(banked, blocks)
                root = banked._bank.root
                assert type(root) is voice_bank._GainNode and type(root.children["gain"]) is voice_bank._AdsrTriggeredNode
                svf = root.children["source"]
                assert type(svf) is voice_bank._SvfNode and type(svf.children["source"]) is voice_bank._NoiseNode
                again = _render_hat(banked, blocks)                              # stop / start: from the seeds again
                _assert_equal(again, got, f"hihat {name}: stop / start")
                _assert_equal(got, _render_hat(_hihat_mix(bank=False), blocks), f"hihat {name} windows={windows}")
                # ... and with look-ahead on, as a user runs it: the per-voice SVFilterPEs then render windows of several
                # blocks -- the same float64 scan in another association, the bar of tests/test_gpu_percussive_bank.py:204
                # (PEAK_BOUND = 1e-6 of the peak) for such a path
                ahead = _render_hat(_hihat_mix(bank=False), blocks, ahead=True)
                assert_peak(f"hihat {name} look-ahead on", np.concatenate(got), np.concatenate(ahead), PEAK_BOUND, "HIHAT")
    finally:
        pg.set_sample_rate(SR)


# ---------------------------------------------------------------------------------------- 5. FunctionGenPE modulators
FG_BLOCKS = [(0, 3077), (3077, 1024), (4101, 1), (4102, 2047), (30000, 1025)]


def _lfo(i):
    return pg.FunctionGenPE(0.7 + 0.31 * i, (0.5, 0.0, 1.0, 0.25)[i % 4], phase=0.1 * i,
                            waveform="sawtooth")


def _pwm_voice(i, wave):
    return pg.AnalogOscPE(109.37 * 2 ** (i / 12), duty_cycle=pg.TransformPE(_lfo(i), func=Affine(0.3, 0.5)), waveform=wave)


def _swept_voice(i, wave=None):
    return pg.BiquadPE(pg.BlitSawPE(109.37 * 2 ** (i / 12)), frequency=pg.TransformPE(_lfo(i), func=Affine(2000.0, 2500.0)),
                       q=2.0)


def _fg_mix(voice, wave, bank=True):
    mix = pg.MixPE(*[voice(i, wave) for i in range(5)])
    if not bank:
        mix._bank = False
    return mix


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("voice,wave,child", [(_pwm_voice, "rectangle", "duty"), (_pwm_voice, "sawtooth", "duty"),
                                              (_swept_voice, None, "frequency")])
def test_voices_modulated_by_a_function_generator(voice, wave, child):
    pg.set_sample_rate(SR)
    with guarded():
        banked = _fg_mix(voice, wave)
        got = _render_blocks(banked, FG_BLOCKS)
        assert banked._bank
        transform = banked._bank.root.children[child]
        level = transform.children["source"]
        assert type(transform) is voice_bank._TransformNode and type(level) is voice_bank._FunctionGenNode and level.k == 5
        _assert_equal(got, _render_blocks(_fg_mix(voice, wave, bank=False), FG_BLOCKS), f"{voice.__name__} {wave}")
        # the modulator level itself: every voice's row is its PE's own render, bit for bit
        for start, n in FG_BLOCKS:
            rows = level.render(start, n).to_host()
            assert rows.shape == (5, n, 1)
            for i in range(5):
                own = _lfo(i).render(start, n).data
                assert np.array_equal(rows[i].view(np.uint32), np.ascontiguousarray(own).view(np.uint32)), (start, n, i)


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("wave", ["rectangle", "sawtooth"])
def test_function_generators_as_sources(wave, channels):
    """A MixPE of FunctionGenPEs (any channel count): one launch, every voice its PE's samples."""
    pg.set_sample_rate(SR)

    def mix(bank=True):
        m = pg.MixPE(*[pg.FunctionGenPE(3.0 + 1.7 * i, 0.2 * i, phase=0.3 * i, waveform=wave, channels=channels)
                       for i in range(6)])
        if not bank:
            m._bank = False
        return m

    with guarded():
        banked = mix()
        got = _render_blocks(banked, FG_BLOCKS)
        assert type(banked._bank.root) is voice_bank._FunctionGenNode and banked._bank.root.channels() == channels
        assert got[0].shape == (FG_BLOCKS[0][1], channels)
        _assert_equal(got, _render_blocks(mix(bank=False), FG_BLOCKS), f"sources {wave} ch={channels}")
