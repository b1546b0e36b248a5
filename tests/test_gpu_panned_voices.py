"""GPU: a MixPE of panned voices -- SpatialPE under SpatialLinear / SpatialConstantPower / SpatialAdapter -- is rendered as
a voice bank (voice_bank._PanNode: pgx_pan_gains once, then pgx_pan_mix_batch as the root or pgx_pan_bank as a level;
_AdaptNode: pgx_channel_adapt over the stacked frames) and gives, bit for bit, what a twin graph rendered voice by voice
(`mix._bank = False`) gives.  Graphs: tests/pan_cases.py, five voices each (the scalar-panned one also at 33: two chunks
of the fused mix).  Pull script: contiguous blocks of 1 024 and of 3 077 frames, a seek back, renderer stop + start.
Mixes that are no bank (HRTF voices, mixed method classes, scalar and PE azimuths mixed, a two-channel azimuth PE, an
azimuth PE shared by two voices) are declined and still equal their twin.  The banked render of the two fixture cases is
held to the reference's samples (tests/golden/panned_mix*, tools/gen_golden_panned_mix.py) by the per-block rule of
graphs with oscillators and filters.  Windows at the level of the mix (the existing rule of a sharded mix's share) hand
out the same samples.  The measured minimums are set to MIN_VOICES.

The two graphs that hold BlitSawPE -> BiquadPE under the pan (`lfo`, `readme`) are compared bit for bit as
tests/test_gpu_voice_bank.py compares such voices: with the oscillator kernels that are bit-identical by construction
(WIDE_SUPERSAW / WIDE_LONG_RENDERS off: the sixteen-frames-per-thread kernels cut a bank and a single voice into time
segments differently, a float32 ulp here and there) and block by block on both paths (look-ahead off, as
tests/test_gpu_noise_bank.py's hi-hat twin: a longer look-ahead window is the same filter recurrence in another
association).  With everything at its default the same two graphs are held to fixture_harness.PEAK_BOUND, the bound
tests/test_gpu_percussive_bank.py holds those paths to."""

import numpy as np
import pytest

import pan_cases
import pygmu2_amd as pg
import spec_build
from fixture_harness import PEAK_BOUND, assert_bits, assert_peak, check_case, load_cases
from guarded_alloc import guarded
from pygmu2_amd import blit_saw_pe, look_ahead, voice_bank

pytestmark = pytest.mark.gpu

SR = pan_cases.SR
# contiguous blocks of 1 024 and of 3 077 frames, a seek back, (stop + start in front of block 6,) two more
PULLS = [(0, 1024), (1024, 1024), (2048, 3077), (5125, 3077), (1024, 1024), (2048, 1024), (0, 3077), (3077, 1024)]
RESTART_AT = 6
DOC, NPZ = load_cases("panned_mix")
FILTERED = ("lfo", "readme")                  # BlitSawPE -> BiquadPE under the pan


@pytest.fixture
def small_banks(monkeypatch):
    for name in ("NOISE_MIN_VOICES", "SVF_MIN_VOICES", "ADSR_TRIGGERED_MIN_VOICES", "ANALOG_OSC_MIN_VOICES",
                 "BIQUAD_VAR_MIN_VOICES"):
        monkeypatch.setattr(voice_bank, name, voice_bank.MIN_VOICES)


@pytest.fixture
def exact_kernels(monkeypatch):
    """The oscillator kernels that are bit-identical between a bank and a single voice, and no look-ahead windows."""
    monkeypatch.setattr(voice_bank, "WIDE_SUPERSAW", False)
    monkeypatch.setattr(blit_saw_pe, "WIDE_LONG_RENDERS", False)
    was = look_ahead.enabled()
    look_ahead.set_enabled(False)
    yield
    look_ahead.set_enabled(was)


def _render(spec, bank, sr=SR):
    """-> (the blocks of the pull script, the MixPE)."""
    pg.set_sample_rate(sr)
    mix = spec_build.build(spec)
    if not bank:
        mix._bank = False
    r = pg.NullRenderer(sample_rate=sr)
    r.set_source(mix)
    r.start()
    out = []
    for k, (start, n) in enumerate(PULLS):
        if k == RESTART_AT:
            r.stop()
            r.start()
        out.append(np.array(mix.render(start, n).data, dtype=np.float32))
    r.stop()
    return out, mix


def _assert_twins(got, want, channels, what):
    assert len(got) == len(want) == len(PULLS)
    for k, (a, b) in enumerate(zip(got, want)):
        assert b.shape == (PULLS[k][1], channels), f"{what} block {k}: {b.shape}"
        assert np.all(np.isfinite(b)) and np.any(b), f"{what} block {k} is silent"
        if channels == 2 and "adapt" not in what:
            assert not np.array_equal(b[:, 0], b[:, 1]), f"{what} block {k}: the channels are equal"
        assert_bits(f"{what} block {k}", a, b)


CASES = [(kind, pan_cases.K) for kind in pan_cases.ROOTS if kind not in FILTERED] + [("scalar", 33)]


def _twins(kind, count):
    """-> (the bank's blocks, the twin's blocks), the bank and its root asserted."""
    spec = pan_cases.mix(kind, count)
    with guarded():
        got, mix = _render(spec, bank=True)
        bank = mix._bank
        assert isinstance(bank, voice_bank.VoiceBank) and bank.k == count
        assert type(bank.root).__name__ == pan_cases.ROOTS[kind]
        if kind in ("lfo", "readme"):
            assert isinstance(bank.root.children["source"], (voice_bank._BiquadNode, voice_bank._GainNode))
        want, plain = _render(spec, bank=False)
        assert plain._bank is False
    return got, want


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("kind,count", CASES, ids=[f"{kind}-{count}" for kind, count in CASES])
def test_bank_equals_the_voices_one_by_one(kind, count):
    got, want = _twins(kind, count)
    _assert_twins(got, want, 1 if kind == "adapt_down" else 2, f"{kind}-{count}")


@pytest.mark.usefixtures("small_banks", "exact_kernels")
@pytest.mark.parametrize("kind", FILTERED)
def test_bank_over_filtered_voices_equals_the_voices_one_by_one(kind):
    got, want = _twins(kind, pan_cases.K)
    _assert_twins(got, want, 2, kind)


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("kind", FILTERED)
def test_bank_over_filtered_voices_at_the_defaults(kind):
    got, want = _twins(kind, pan_cases.K)
    assert_peak(f"{kind}, defaults", np.concatenate(got), np.concatenate(want), PEAK_BOUND, "PANNED_DEFAULT")


@pytest.mark.parametrize("kind", ["scalar", "nested"])
def test_windows_of_the_mix_hand_out_the_block_by_block_samples(kind):
    """The existing window rule of a rank's share of a sharded mix (VoiceBank.set_mix_windows) over a pan root and over a
    pan level: a stream of 4 096-frame blocks is rendered 2, then 4 blocks at a time -- one pgx_pan_mix_batch per window --,
    a seek leaves the window of 4 half consumed.  Stateless voices, so the rows are the twin's blocks bit for bit."""
    pulls = [(4096 * i, 4096) for i in range(5)] + [(4096, 4096), (8192, 4096)]
    spec = pan_cases.mix(kind)
    pg.set_sample_rate(SR)
    with guarded():
        out = {}
        for name in ("bank", "twin"):
            mix = spec_build.build(spec)
            r = pg.NullRenderer(sample_rate=SR)
            r.set_source(mix)
            r.start()
            if name == "bank":
                assert mix._voice_bank()
                mix._bank.set_mix_windows()
            else:
                mix._bank = False
            out[name], windows = [], []
            for start, n in pulls:
                out[name].append(np.array(mix.render(start, n).data, dtype=np.float32))
                windows.append(bool(mix._bank) and mix._bank.win is not None)
            r.stop()
            if name == "bank":
                assert windows == [False, True, True, True, True, False, True], windows     # 2, 4, the seek, 2 again
    for k, (a, b) in enumerate(zip(out["bank"], out["twin"])):
        assert b.shape == (4096, 2) and np.any(b) and not np.array_equal(b[:, 0], b[:, 1])
        assert_bits(f"{kind} block {k}", a, b)


@pytest.mark.usefixtures("small_banks")
def test_fused_root_off_is_the_same_samples(monkeypatch):
    """FUSED_PAN_MIX = False: pgx_pan_bank + pgx_mix_batch, what tools/pan_bank_probe.py compares the fused root with.
    (Two banks: the same kernels under the pan, whatever the switches.)"""
    spec = pan_cases.mix("lfo")
    with guarded():
        fused, _ = _render(spec, bank=True)
        monkeypatch.setattr(voice_bank, "FUSED_PAN_MIX", False)
        layered, mix = _render(spec, bank=True)
        assert isinstance(mix._bank, voice_bank.VoiceBank)
    _assert_twins(layered, fused, 2, "lfo, layered")


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("kind", pan_cases.DECLINED)
def test_declined_mixes_still_equal_their_twin(kind):
    spec = pan_cases.declined(kind)
    sr = 44100 if kind == "hrtf" else SR                          # (the KEMAR set's rate)
    with guarded():
        got, mix = _render(spec, bank=True, sr=sr)
        assert mix._bank is False
        want, _ = _render(spec, bank=False, sr=sr)
    _assert_twins(got, want, 2, kind)


@pytest.mark.usefixtures("small_banks")
@pytest.mark.parametrize("case", DOC["cases"], ids=[c["name"] for c in DOC["cases"]])
def test_bank_matches_the_reference(case):
    assert case["compare"] == "fuzz"
    built = []

    def build(case):
        pe, made = spec_build.build_case(case, ())
        built.append(pe)
        return pe, made

    check_case(case, NPZ, build, tag="PANNED_MIX_ERR")
    bank = built[0]._bank
    assert isinstance(bank, voice_bank.VoiceBank) and type(bank.root) is voice_bank._PanNode and bank.k == pan_cases.K
