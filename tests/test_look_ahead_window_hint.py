"""CPU: the size of a look-ahead window when its root has a figure of its own.  look_ahead.window_blocks over a grid (no hint:
the formula render used before; a smaller hint binds; never fewer than 2 blocks; an explicit PGX_LOOK_AHEAD_FRAMES wins),
pgx_biquad_tone_window_frames without a device and under PGX_TONE_WINDOW_FRAMES (read once: fresh child processes), and
the conditions under which BiquadPE hands the figure on."""

import itertools
import os
import subprocess
import sys

import pytest

from pygmu2_amd import biquad_pe, device, look_ahead
from pygmu2_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROWS = [8, 16, 32, 64, 128, 256, 1 << 20]
DURATIONS = [1, 1024, 44_100, 999_999, 1_000_000, 1 << 20]
NODES = [1, 2, 3, 4, 5, 40]
HINTS = [None, 0, 1, 1_000_000, 17_000_000, 36_000_000, 1 << 25, 1 << 27, 1 << 40]


@pytest.fixture(scope="module")
def lib():
    build()
    return device.load_library()


def _before(grow, duration, n_nodes):
    """The expression look_ahead.render held before window_blocks was factored out of it."""
    return max(2, min(grow, look_ahead.AHEAD_BLOCKS, look_ahead.frame_cap(n_nodes) // duration))


def test_window_blocks_over_the_grid(monkeypatch):
    monkeypatch.setattr(look_ahead, "_FRAMES_EXPLICIT", False)
    monkeypatch.setattr(look_ahead, "AHEAD_BLOCKS", 256)
    monkeypatch.setattr(look_ahead, "AHEAD_FRAMES", 1 << 25)
    monkeypatch.setattr(look_ahead, "AHEAD_FRAMES_SMALL_GRAPH", 1 << 27)
    bound = 0
    for grow, duration, nodes in itertools.product(GROWS, DURATIONS, NODES):
        plain = _before(grow, duration, nodes)
        assert look_ahead.window_blocks(grow, duration, nodes) == plain
        assert look_ahead.window_blocks(grow, duration, nodes, None) == plain
        assert look_ahead.window_blocks(grow, duration, nodes, 0) == plain          # 0: no preference
        for hint in HINTS[2:]:
            got = look_ahead.window_blocks(grow, duration, nodes, hint)
            assert got == max(2, min(plain, hint // duration))
            assert 2 <= got <= plain
            assert got * duration <= max(look_ahead.frame_cap(nodes), 2 * duration)
            if hint // duration >= 2:
                assert got * duration <= hint
            bound += got < plain
    assert bound > 100                                       # the grid does reach hints that bind
    # the stream the benchmark renders: 1 M-frame blocks under a two-PE root, with a 36 M-frame hint and without
    assert [look_ahead.window_blocks(g, 1_000_000, 2, 36_000_000) for g in (8, 16, 32, 64, 128)] == [8, 16, 32, 36, 36]
    assert [look_ahead.window_blocks(g, 1_000_000, 2) for g in (8, 16, 32, 64, 128, 256)] == [8, 16, 32, 64, 128, 134]


def test_an_explicit_frame_cap_wins(monkeypatch):
    monkeypatch.setattr(look_ahead, "_FRAMES_EXPLICIT", True)
    for cap in (1 << 24, 1 << 25, 67_000_000):
        monkeypatch.setattr(look_ahead, "AHEAD_FRAMES", cap)
        for grow, duration, nodes, hint in itertools.product(GROWS, DURATIONS, NODES, HINTS):
            assert look_ahead.window_blocks(grow, duration, nodes, hint) == _before(grow, duration, nodes)
        assert look_ahead.window_blocks(256, 1_000_000, 2, 17_000_000) == min(256, cap // 1_000_000)


def test_the_native_figure_needs_no_device(lib):
    if "PGX_TONE_WINDOW_FRAMES" not in os.environ:
        frames = lib.pgx_biquad_tone_window_frames()
        # a hint can only shorten a window: a figure beyond the largest cap would never bind.  The smallest size class
        # the closed-form kernel takes is 16 M frames
        assert 16_000_000 <= frames <= 1 << 27
        assert biquad_pe.tone_window_frames() == frames
    assert lib.pgx_biquad_tone_window_frames() == lib.pgx_biquad_tone_window_frames()


@pytest.mark.parametrize("value, want", [("17000000", 17_000_000), ("0", 0), ("134217728", 134_217_728), (None, None),
                                         ("", None), ("many", None), ("-5", None)])
def test_the_override_is_read_in_a_fresh_process(lib, value, want):
    """PGX_TONE_WINDOW_FRAMES replaces the built-in figure, 0 (no preference) included; what is no count leaves it."""
    env = {k: v for k, v in os.environ.items() if k != "PGX_TONE_WINDOW_FRAMES"}
    code = ("import ctypes; from pygmu2_amd.build import LIB_PATH; L = ctypes.CDLL(LIB_PATH); "
            "L.pgx_biquad_tone_window_frames.restype = ctypes.c_int64; print(L.pgx_biquad_tone_window_frames())")
    built_in = int(subprocess.check_output([sys.executable, "-c", code], env=env, cwd=ROOT, text=True))
    assert built_in > 0
    if value is not None:
        env["PGX_TONE_WINDOW_FRAMES"] = value
    got = int(subprocess.check_output([sys.executable, "-c", code], env=env, cwd=ROOT, text=True))
    assert got == (built_in if want is None else want)


class _Lib:
    """The two questions _look_ahead_frames asks: the wave-run plan (device-sized: answered here) and the gate (the real one)."""

    def __init__(self, real, window_from=16_000_000):
        self.real, self.window_from = real, window_from

    def pgx_biquad_sine_runs_plan(self, n, settle, out):
        return 1 if n >= self.window_from else 0

    def pgx_biquad_tone_supported(self, *args):
        return self.real.pgx_biquad_tone_supported(*args)


def _pe(monkeypatch, lib, tone, cutoff, mode, frames=30_000_000, **sine):
    import pygmu2_amd as pg
    from pygmu2_amd.biquad_pe import BiquadMode, rbj_coefficients, settle_frames
    pg.set_sample_rate(44100)
    pe = pg.BiquadPE(pg.SinePE(frequency=tone, **sine), frequency=cutoff, q=0.707, mode=BiquadMode(mode))
    pe._coef_host = rbj_coefficients(BiquadMode(mode), cutoff, 0.707, 0.0, 44100.0)
    pe._settle = settle_frames(pe._coef_host[3], pe._coef_host[4])
    pe._coef = object()                                      # _prepare_constant: the constants are in place
    monkeypatch.setattr(biquad_pe, "lib", lambda: _Lib(lib))
    monkeypatch.setattr(biquad_pe, "tone_window_frames", lambda: frames)
    return pe


def test_biquad_pe_hands_the_figure_on_only_for_tone_windows(lib, monkeypatch):
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", True)
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass")._look_ahead_frames() == 30_000_000
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass", frames=17_000_000)._look_ahead_frames() == 17_000_000
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass", frames=0)._look_ahead_frames() is None      # no preference
    # a figure below the sizes the window kernels take is no window of theirs
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass", frames=8_000_000)._look_ahead_frames() is None
    # the gate declines the chain (55 Hz into an 8 kHz high-pass); a stereo sine is not the fused chain
    assert _pe(monkeypatch, lib, 55.0, 8000.0, "highpass")._look_ahead_frames() is None
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass", channels=2)._look_ahead_frames() is None
    # PYGMU_BIQUAD_TONE=0, also when it is switched off after the figure was asked for once
    pe = _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass")
    assert pe._look_ahead_frames() == 30_000_000
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", False)
    assert pe._look_ahead_frames() is None
    assert _pe(monkeypatch, lib, 440.0, 1000.0, "lowpass")._look_ahead_frames() is None


def test_other_roots_have_no_figure():
    import pygmu2_amd as pg
    assert not hasattr(pg.SinePE(frequency=440.0), "_look_ahead_frames")
    assert not hasattr(pg.GainPE(pg.SinePE(frequency=440.0), gain=0.5), "_look_ahead_frames")
