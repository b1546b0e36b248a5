"""CPU: the host side of the closed-form BiquadPE(SinePE) window (csrc/pgx_tone.hip).  pgx_biquad_tone_supported is a host
computation: its |H| and sum|h| against numpy for the five chains of the issue's table, its conditions one by one, and
the choice BiquadPE makes between the closed form and the wave-run kernel (switch on, switch off, chain declined)."""

import numpy as np
import pytest

from pygmu2_amd import biquad_pe, device
from pygmu2_amd.biquad_pe import BiquadMode, rbj_coefficients, settle_frames
from pygmu2_amd.build import build

SR = 44100.0
#          tone Hz, cutoff, q, mode, gain dB, sum|h| / |H| of the issue's table
CHAINS = [(440.0, 1000.0, 0.707, "lowpass", 0.0, 1.11), (3000.3, 2500.0, 2.0, "bandpass", 0.0, 1.60),
          (5500.0, 3000.0, 0.707, "highpass", 0.0, 1.99), (700.0, 1000.0, 1.0, "peaking", 6.0, 1.46),
          (55.0, 8000.0, 0.707, "highpass", 0.0, 3.6e4)]


@pytest.fixture(scope="module")
def lib():
    build()
    return device.load_library()


def _numpy_gain_l1(c, omega, frames):
    z1 = np.exp(-1j * omega)
    gain = abs((c[0] + c[1] * z1 + c[2] * z1 * z1) / (1.0 + c[3] * z1 + c[4] * z1 * z1))
    from scipy.signal import lfilter
    x = np.zeros(frames)
    x[0] = 1.0
    return gain, float(np.sum(np.abs(lfilter(c[:3], [1.0, c[3], c[4]], x))))


@pytest.mark.parametrize("tone, cutoff, q, mode, gain_db, ratio", CHAINS)
def test_gain_and_l1_against_numpy(lib, tone, cutoff, q, mode, gain_db, ratio):
    c = rbj_coefficients(BiquadMode(mode), cutoff, q, gain_db, SR)
    settle = settle_frames(c[3], c[4])
    w = 2.0 * np.pi * tone
    gain, l1 = _numpy_gain_l1(c, w / SR, settle)
    got_gain, got_l1 = lib.pgx_biquad_tone_gain(w, SR, *c), lib.pgx_biquad_tone_l1(settle, *c)
    assert abs(got_gain - gain) <= 1e-12 * max(gain, 1e-3), (got_gain, gain)
    assert abs(got_l1 - l1) <= 1e-12 * l1, (got_l1, l1)
    assert abs(got_l1 / got_gain / ratio - 1.0) <= 0.02                     # the issue's table, two or three digits
    assert lib.pgx_biquad_tone_supported(134_000_000, settle, w, SR, *c) == (1 if ratio <= 4.0 else 0)


def test_conditions_one_by_one(lib):
    c = rbj_coefficients(BiquadMode.LOWPASS, 1000.0, 0.707, 0.0, SR)
    settle, w = settle_frames(c[3], c[4]), 2.0 * np.pi * 440.0
    assert settle == 1024
    ok = lambda n, s=settle, ww=w: lib.pgx_biquad_tone_supported(n, s, ww, SR, *c)
    assert ok(134_000_000) == 1 and ok(2 * settle) == 1
    assert ok(2 * settle - 1) == 0                                           # n < 2 settle_frames
    assert ok(134_000_000, 0) == 0                                           # a section that does not forget
    assert ok(134_000_000, 8192) == 0                                        # its response outlasts workgroup 0's piece
    assert ok(134_000_000, settle, 2.0 * np.pi * 20_000.0 * 60.0) == 0       # |w| n / sr beyond the fast sine's range
    # the bound itself: a 3 kHz high-pass takes a 5.5 kHz tone and declines a 400 Hz one, which it passes 35 dB down
    hp = rbj_coefficients(BiquadMode.HIGHPASS, 3000.0, 0.707, 0.0, SR)
    s = settle_frames(hp[3], hp[4])
    r = lambda f: lib.pgx_biquad_tone_l1(s, *hp) / lib.pgx_biquad_tone_gain(2.0 * np.pi * f, SR, *hp)
    for f in (400.0, 1000.0, 2000.0, 5500.0):
        assert lib.pgx_biquad_tone_supported(10 ** 6, s, 2.0 * np.pi * f, SR, *hp) == (1 if r(f) <= 4.0 else 0)
    assert r(400.0) > 4.0 > r(5500.0)


class _Lib:
    """The two questions _takes_tone_window asks: the wave-run plan (device-sized: answered here) and the gate (the real one)."""

    def __init__(self, real, window_from):
        self.real, self.window_from, self.asked = real, window_from, []

    def pgx_biquad_sine_runs_plan(self, n, settle, out):
        self.asked.append(n)
        return 1 if n >= self.window_from else 0

    def pgx_biquad_tone_supported(self, *args):
        return self.real.pgx_biquad_tone_supported(*args)


def _pe(tone, cutoff, mode):
    import pygmu2_amd as pg
    pg.set_sample_rate(int(SR))
    pe = pg.BiquadPE(pg.SinePE(frequency=tone), frequency=cutoff, q=0.707, mode=BiquadMode(mode))
    pe._coef_host = rbj_coefficients(BiquadMode(mode), cutoff, 0.707, 0.0, SR)
    pe._settle = settle_frames(pe._coef_host[3], pe._coef_host[4])
    return pe


def test_the_choice_in_biquad_pe(lib, monkeypatch):
    L = _Lib(lib, 16_000_000)
    w = 2.0 * np.pi * 440.0
    pe = _pe(440.0, 1000.0, "lowpass")
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", True)
    assert pe._takes_tone_window(L, 0, 134_000_000, w, 0.0, SR) is True
    assert pe._takes_tone_window(L, 10 ** 9, 134_000_000, w, 0.0, SR) is True
    assert L.asked == [134_000_000]                                          # asked once per size
    assert pe._takes_tone_window(L, 0, 1_000_000, w, 0.0, SR) is False       # not window-sized: as before
    assert pe._takes_tone_window(L, 4 * 10 ** 10, 134_000_000, w, 0.0, SR) is False     # phase beyond the fast sine's range
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", False)                    # PYGMU_BIQUAD_TONE=0
    assert pe._takes_tone_window(L, 0, 134_000_000, w, 0.0, SR) is False
    monkeypatch.setattr(biquad_pe, "TONE_WINDOWS", True)
    low = _pe(55.0, 8000.0, "highpass")                                      # declined by the gate
    assert low._takes_tone_window(L, 0, 134_000_000, 2.0 * np.pi * 55.0, 0.0, SR) is False
