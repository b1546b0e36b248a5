"""GPU: TralfamPE, SlicePE and SetExtentPE on the device against the reference-rendered fixtures
(tests/golden/tralfam_cases.json + tralfam.npz, tools/gen_golden_tralfam.py).

Bounds (set before any device run): a TralfamPE case max abs error <= 1e-6 * peak of the case -- the project's class
for re-associated float64 sums rounded to float32; the reference itself lies within 1.8e-7 * peak of a float64
restatement (its forward transform is complex64) -- and exactly zero where the peak is 0; SetExtentPE and SlicePE
without fades bit for bit; SlicePE with fades the GainPE class of tests/test_gpu_fuzz.py (1e-5 * peak + 1e-6 per block).
Every stored sample is compared; every length runs once."""

import numpy as np
import pytest

import pygmu2_amd as pg
import tralfam_oracle as T
from fixture_harness import PEAK_BOUND, load_cases, max_err
from tralfam_gpu_common import check_case

pytestmark = pytest.mark.gpu

CASES, NPZ = load_cases("tralfam")
ALL = CASES["cases"]


class ProbePE(pg.ArrayPE):
    """An ArrayPE that records every (start, duration) its _render is asked for."""

    def __init__(self, data):
        super().__init__(data)
        self.pulls = []

    def _render(self, start, duration):
        self.pulls.append((start, duration))
        return super()._render(start, duration)


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_case_matches_reference(case):
    check_case(case, NPZ)


def test_source_is_pulled_once_for_the_whole_extent():
    pg.set_sample_rate(48000)
    x = T.make_signal({"kind": "noise_decay", "n": 5000}, None)
    probe = ProbePE(x)
    t = pg.TralfamPE(pg.DelayPE(probe, 300), seed=5)
    whole = t.render(300, 5000).data.copy()
    assert probe.pulls == [(0, 5000)]
    for start in range(-1000, 7000, 1000):                       # outside, across either edge, inside
        block = t.render(start, 1000).data
        lo, hi = max(start, 300), min(start + 1000, 5300)
        want = np.zeros((1000, 1), dtype=np.float32)
        if hi > lo:
            want[lo - start:hi - start] = whole[lo - 300:hi - 300]
        assert np.array_equal(block, want), start
    assert probe.pulls == [(0, 5000)]
    # a pure graph over a pure source pulled in small sequential blocks opens read-ahead windows: still the one pull
    probe = ProbePE(x)
    g = pg.GainPE(pg.TralfamPE(probe, seed=5), 0.5)
    got = np.concatenate([g.render(s, 100).data for s in range(-200, 6400, 100)])
    want = np.zeros((6600, 1), dtype=np.float32)
    want[200:5200] = whole * np.float32(0.5)
    assert np.array_equal(got, want)
    assert "_ra_win" in g.__dict__                                # a window did open
    assert probe.pulls == [(0, 5000)]


def test_first_render_outside_the_extent_pulls_the_whole_extent():
    pg.set_sample_rate(48000)
    probe = ProbePE(T.make_signal({"kind": "ramp", "n": 640}, None))
    t = pg.TralfamPE(probe, seed=1)
    assert not np.any(t.render(10_000, 64).data)                 # the reference mogrifies before the overlap test
    assert probe.pulls == [(0, 640)]


def test_seed_none_draws_fresh_entropy_per_instance():
    pg.set_sample_rate(48000)
    x = T.make_signal({"kind": "noise_decay", "n": 2048}, None)
    a = pg.TralfamPE(pg.ArrayPE(x)).render(0, 2048).data
    b = pg.TralfamPE(pg.ArrayPE(x)).render(0, 2048).data
    assert np.any(a) and np.any(b) and not np.array_equal(a, b)
    # the magnitudes are the source's either way
    mag = np.abs(np.fft.fft(x[:, 0].astype(np.float64)))
    for y in (a, b):
        assert float(np.max(np.abs(y))) <= float(np.sum(mag)) / 2048 * (1 + 1e-6)
    c = pg.TralfamPE(pg.ArrayPE(x), seed=11).render(0, 2048).data
    d = pg.TralfamPE(pg.ArrayPE(x), seed=11).render(0, 2048).data
    assert np.array_equal(c, d)


def test_normalize_peak_lands_on_the_float32_quotient():
    pg.set_sample_rate(48000)
    x = T.make_signal({"kind": "noise_decay", "n": 3001, "channels": 2}, None)
    plain = pg.TralfamPE(pg.ArrayPE(x), seed=2).render(0, 3001).data
    scaled = pg.TralfamPE(pg.ArrayPE(x), seed=2, normalize_peak=0.3).render(0, 3001).data
    peak = np.max(np.abs(plain))
    assert np.array_equal(scaled, plain * (np.float32(0.3) / peak))      # the same float32 quotient and product


def test_extent_past_the_limit_is_a_value_error():
    pg.set_sample_rate(48000)
    limit = pg.spectral.max_length()
    src = pg.SetExtentPE(pg.ArrayPE(np.ones(16, dtype=np.float32)), 0, limit + 1)
    with pytest.raises(ValueError, match=str(limit)):
        pg.TralfamPE(src, seed=1).render(0, 16)
    ok = pg.SetExtentPE(pg.ArrayPE(np.ones(16, dtype=np.float32)), 0, 4097)
    assert pg.TralfamPE(ok, seed=1).render(0, 4097).data.shape == (4097, 1)


def test_device_matches_the_bluestein_model_through_the_pe():
    """The PE's whole pipeline against the numpy model of the device algorithm (Bluestein over np.fft, the modelled
    draws), not only against the float64 restatement."""
    pg.set_sample_rate(48000)
    n, seed = 1531, 12345
    x = T.make_signal({"kind": "noise_decay", "n": n}, None)
    mag = np.abs(T.bluestein_dft(x[:, 0].astype(np.float64)))
    phi = (T.model_random(seed, 0, n) * 2.0) * np.pi
    want = np.real(T.bluestein_dft(mag * np.exp(1j * phi), inverse=True)).astype(np.float32).reshape(-1, 1)
    got = pg.TralfamPE(pg.ArrayPE(x), seed=seed).render(0, n).data
    peak = float(np.max(np.abs(want)))
    err = max_err(got, want)
    print(f"TRALFAM_ERR model n={n} max_abs_err={err:.3e} peak={peak:.3e}")
    assert err <= PEAK_BOUND * peak
